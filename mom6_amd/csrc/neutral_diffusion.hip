// neutral_diffusion.hip -- the continuous-reconstruction branch of MOM_neutral_diffusion (src/tracer/MOM_neutral_diffusion.F90)
// as gfx950 kernels, called from tracer_hordiff's neutral branch (MOM_tracer_hor_diff.F90:474-534; tracer_hor_diff.hip).
//
//   nd_column_kernel      neutral_diffusion_calc_coeffs :337-470 for one h column (halo 1): interface pressures, interface T and S by
//                         interface_scalar (:1078, PLM_diff + ppm_edge), their density derivatives -> one record of five numbers an interface
//   nd_surfaces_kernel    find_neutral_surface_positions_continuous (:1353) for one face: the merge walk down the 2nk+2 interfaces of
//                         the two columns; PoL, PoR, KoL, KoR, hEff (back in H units, :570-575) as [surface][face] planes
//   nd_tracer_cols_kernel interface values of a batch of up to 4 tracers (neutral_surface_flux :2373-2374) for one h column, with the means
//                         of the cells: one record of eight numbers an interface
//   nd_flux_kernel        neutral_surface_flux (:2297) for one face and the batch.  With the sums in the symmetric order
//                         (NDIFF_ANSWER_DATE > 20240330, :939-954: a face at a time) the kernel leaves the tendencies of the layers of the
//                         two cells of the face -- a surface never lies above the one before it, so a layer's sum is a run of consecutive
//                         surfaces and is kept in a register -- and nd_update_sym_kernel adds the four faces of a cell and updates the
//                         tracer (:955-959).  With the older order (:927-938: surface by surface round the four faces) it leaves the
//                         fluxes [surface][face] and nd_update_kernel accumulates them per layer in LDS.
//   nd_coef_h_kernel      KHTR_USE_EBT_STRUCT: Coef_h (neutral_diffusion :670-684) of a wet column of the compute domain, straight from
//                         khdt_x / khdt_y, I_numitts and VarMix%ebt_struct (the interface coefficients of MOM_tracer_hor_diff.F90:489-518
//                         are formed in registers), as planes [interface][h points]; its halo is a group pass
//   nd_taper_kernel       NDIFF_TAPERING: the four layer numbers of compute_tapering_coeffs (:1022) for one face -- boundary_k_range of
//                         the two columns at the smaller and the larger of their boundary-layer depths; coeff_l / coeff_r are closed
//                         forms of them
//   nd_trans_march_kernel, and the forms of the flux and update kernels that take a record  the diagnostics neutral_diffusion posts
//                         (:935-1014: dfx_2d, dfy_2d, dfxy_cont, dfxy_cont_2d, dfxy_conc) where mom6hip_tracer_hordiff_mix_diag asks for them
// With either switch nd_flux_kernel forms khtr_ave (:2410-2417) from the coefficients of the interfaces klt, klb, krt, krb: a side's value
// at klt is its value at klb of the sublayer above, so one is carried and a new one is formed only when the surface enters another cell.
// A lane owns a column or a face and walks it: the walks are serial in the surface index and differ from lane to lane.  What a walk
// reads at a depth of its own (the interfaces of a column) is stored as records, so that a gather is one or two sectors and not one a
// number, and kept in registers while the walk stays in the cell: a step down a column loads one record.  What all lanes read at the
// same step (the surfaces of a face) is stored as planes.  A row of the grid is nbx blocks of 64 lanes along i (nd_face, nd_column).
// What the branch shares with the discontinuous one is neutral_common.hpp; neutral_drive, the host driver of both, is below beside the
// update kernels, which finish the step of either.
#include <cfloat>
#include <cmath>
#include <type_traits>

#include "neutral_common.hpp"
#include "flux_diag_march.hpp"
#include "eos.hpp"

namespace {

using namespace m6;
using namespace m6::eos;

__device__ __forceinline__ double fsign(double a, double b) { return copysign(fabs(a), b); }
__device__ __forceinline__ double signum(double a, double x) { return (x == 0.) ? 0. : fsign(a, x); }      // :1200

// fv_diff :1282
__device__ __forceinline__ double fv_diff(double hkm1, double hk, double hkp1, double Skm1, double Sk, double Skp1) {
  double h_sum = (hkm1 + hkp1) + hk;
  if (h_sum != 0.) h_sum = 1. / h_sum;
  double hm = hkm1 + hk;
  if (hm != 0.) hm = 1. / hm;
  double hp = hkp1 + hk;
  if (hp != 0.) hp = 1. / hp;
  return (hk * h_sum) * ((2. * hkm1 + hk) * hp * (Skp1 - Sk) + (2. * hkp1 + hk) * hm * (Sk - Skm1));
}

// PLM_diff :1211 with c_method = 2, b_method = 1, for an interior layer from its own and its two neighbours' thicknesses and values
__device__ __forceinline__ double plm_diff(double hkm1, double hk, double hkp1, double Skm1, double Sk, double Skp1) {
  if (!((hkp1 + hk) * (hkm1 + hk) > 0.)) return 0.;
  const double diff_c = fv_diff(hkm1, hk, hkp1, Skm1, Sk, Skp1);
  const double diff_l = 2. * (Sk - Skm1), diff_r = 2. * (Skp1 - Sk);
  if (signum(1., diff_l) * signum(1., diff_r) <= 0.) return 0.;
  return fsign(min2(min2(fabs(diff_l), fabs(diff_c)), fabs(diff_r)), diff_c);
}

// ppm_edge :1120
__device__ __forceinline__ double ppm_edge(double hkm1, double hk, double hkp1, double hkp2, double Ak, double Akp1, double Pk, double Pkp1,
                                           double h_neglect) {
  double R_hk_hkp1 = hk + hkp1, e;
  if (R_hk_hkp1 <= 0.) return 0.5 * (Ak + Akp1);
  R_hk_hkp1 = 1. / R_hk_hkp1;
  if (hk < hkp1) e = Ak + (hk * R_hk_hkp1) * (Akp1 - Ak);
  else e = Akp1 + (hkp1 * R_hk_hkp1) * (Ak - Akp1);
  const double R_2hk_hkp1 = 1. / ((2. * hk + hkp1) + h_neglect);
  const double R_hk_2hkp1 = 1. / ((hk + 2. * hkp1) + h_neglect);
  const double f1 = 1. / ((hk + hkp1) + (hkm1 + hkp2));
  const double f2 = 2. * (hkp1 * hk) * R_hk_hkp1 * ((hkm1 + hk) * R_2hk_hkp1 - (hkp2 + hkp1) * R_hk_2hkp1);
  const double f3 = hk * (hkm1 + hk) * R_2hk_hkp1;
  const double f4 = hkp1 * (hkp1 + hkp2) * R_hk_2hkp1;
  return e + f1 * (f2 * (Akp1 - Ak) - (f3 * Pkp1 - f4 * Pk));
}

// interface_scalar :1078 with i_method = 2 for NZ fields of one column, walked down the interfaces K = 0 .. nk: out(K, v, m) gets the
// interface values v[z] and the means m[z] of the cell below the interface (0 at K = nk).  The walk keeps the four thicknesses and three
// values an interface reads in registers and loads one new layer a step (the reference's expressions on the same numbers).
template <int NZ, typename F>
__device__ __forceinline__ void walk_interfaces(const double *__restrict__ h, const double *const *S, int nz, long n2, long hpl, int nk,
                                                double h_neglect, F out) {
  const int k2 = (2 < nk - 1) ? 2 : nk - 1;
  double hB = h[n2], hC = h[n2 + hpl], hD = h[n2 + hpl * k2], hA = hB;
  double sB[NZ], sC[NZ], sD[NZ], dp[NZ], v[NZ];
#pragma unroll
  for (int z = 0; z < NZ; z++) {
    sB[z] = sC[z] = sD[z] = 0.; dp[z] = 0.;      // plm_diff of the top layer is 0
    if (z < nz) { sB[z] = S[z][n2]; sC[z] = S[z][n2 + hpl]; sD[z] = S[z][n2 + hpl * k2]; }
  }
#pragma unroll
  for (int z = 0; z < NZ; z++) v[z] = sB[z] - 0.5 * dp[z];
  out(0, v, sB);
  for (int K = 1; K < nk; K++) {      // hA, hB, hC, hD = h(max(K-2, 0)), h(K-1), h(K), h(min(K+1, nk-1)); sB, sC, sD = S(K-1), S(K), S(min(K+1, nk-1))
#pragma unroll
    for (int z = 0; z < NZ; z++) {
      const double d = (K < nk - 1) ? plm_diff(hB, hC, hD, sB[z], sC[z], sD[z]) : 0.;
      v[z] = ppm_edge(hA, hB, hC, hD, sB[z], sC[z], dp[z], d, h_neglect);
      dp[z] = d;
    }
    out(K, v, sC);
    const int kn = (K + 2 < nk - 1) ? K + 2 : nk - 1;
    hA = hB; hB = hC; hC = hD; hD = h[n2 + hpl * kn];
#pragma unroll
    for (int z = 0; z < NZ; z++) { sB[z] = sC[z]; sC[z] = sD[z]; if (z < nz) sD[z] = S[z][n2 + hpl * kn]; }
  }
  double zero[NZ];
#pragma unroll
  for (int z = 0; z < NZ; z++) { v[z] = sB[z] + 0.5 * dp[z]; zero[z] = 0.; }
  out(nk, v, zero);
}

// interpolate_for_nondim_position :1563
__device__ __forceinline__ double interp_nondim(double dRhoNeg, double Pneg, double dRhoPos, double Ppos) {
  if (Ppos <= Pneg) return 0.5;
  if (dRhoPos - dRhoNeg > 0.) return min2(1., max2(0., -dRhoNeg / (dRhoPos - dRhoNeg)));
  if (dRhoPos - dRhoNeg == 0) {
    if (dRhoNeg > 0.) return 0.;
    if (dRhoNeg < 0.) return 1.;
    return 0.5;
  }
  return 0.5;
}

// ppm_ave :1166
__device__ __forceinline__ double ppm_ave(double xL, double xR, double aL, double aR, double aMean, int &bad) {
  const double dx = xR - xL;
  const double xave = 0.5 * (xR + xL);
  const double a6o3 = 2. * aMean - (aL + aR);
  const double a6 = 3. * a6o3;
  if (dx < 0. || dx > 1.) { bad = 1; return 0.; }
  if (dx == 0.) return aL + (aR - aL) * xR + a6 * xR * (1. - xR);
  return (aL + xave * ((aR - aL) + a6)) - a6o3 * (xR * xR + xR * xL + xL * xL);
}

// ppm_left_right_edge_values :2541 for one cell: the interface values above and below it and its mean
__device__ __forceinline__ void ppm_edges(double Ti0, double Ti1, double Tl, double &aL, double &aR) {
  aL = Ti0; aR = Ti1;
  if (signum(1., aR - Tl) * signum(1., Tl - aL) <= 0.0) { aL = Tl; aR = Tl; }
  else if (fsign(3., aR - aL) * ((Tl - aL) + (Tl - aR)) > fabs(aR - aL)) aL = Tl + 2.0 * (Tl - aR);
  else if (fsign(3., aR - aL) * ((Tl - aL) + (Tl - aR)) < -fabs(aR - aL)) aR = Tl + 2.0 * (Tl - aL);
}

constexpr int IREC = 5;      // an interface of a column: P, T, S, drho/dT, drho/dS
// where field q of interface K (0-based) of the column c is: planes [field][K][h points] (the columns of a wave stand at nearly the same
// depth of their walks: a load of the wave is a few lines; records [K][h points][field] were slower, profiles/r04_experiments.txt)
__device__ __forceinline__ long irec_at(long K, long c, int q, long hpl, int nk) { return ((long)q * (nk + 1) + K) * hpl + c; }
constexpr int TREC = 2 * ND_BATCH;      // an interface of a column for a batch of tracers: their interface values, the means of the cell below

struct NDArgs : NDFaces {
  EosDev E;
  double ref_pres, gH;              // NDIFF_REF_PRES ; GV%g_Earth*GV%H_to_RZ
  double pa_to_H, h_neglect;
  const double *T, *S, *p_surf;
  int interior;                     // NDIFF_INTERIOR_ONLY
  const double *hbl;                // the boundary-layer depth visc%h_ML with its halo (interior)
  int *kbot; double *zbot;          // boundary_k_range of every column: the layer and the fraction of it the boundary layer ends in
  double *irec;                     // [IREC][(nk+1)][h points]: the interfaces of the columns (irec_at)
  double *trec;                     // [(nk+1)][h points][TREC]: interface values and cell means of the batch's tracers
  const double *ebt;                // KHTR_USE_EBT_STRUCT: VarMix%ebt_struct [layer][h points] (null: off)
  double *coef_h;                   // Coef_h [(nk+1)][h points]
  ko_t *kt[2];                      // NDIFF_TAPERING: [k_min_l, k_max_l, k_min_r, k_max_r][faces of the direction] (null: off)
};

__global__ __launch_bounds__(64) void nd_column_kernel(NDArgs A, int nbx) {
  const m6::GridDev &g = A.g;
  const NDCol C = nd_column(g, nbx);
  if (!C.has) return;
  const long n2 = C.n2, hpl = C.hpl;
  const int nk = g.nk;
  if (A.interior) {      // boundary_k_range(SURFACE, ...), src/tracer/MOM_hor_bnd_diffusion.F90:609-647, for wet columns (:381-386)
    int k_bot = 1;
    double zeta_bot = 0.;
    if (g.mask2dT[n2] > 0.0) boundary_k_range_surface(A.h + n2, hpl, nk, A.hbl[n2], k_bot, zeta_bot);
    A.kbot[n2] = k_bot; A.zbot[n2] = zeta_bot;
  }
  double P = A.p_surf ? A.p_surf[n2] : 0.;
  const double *TS[2] = {A.T, A.S};
  double h_above = 0.;
  walk_interfaces<2>(A.h, TS, 2, n2, hpl, nk, A.h_neglect, [&](int K, const double *v, const double *m) {
    (void)m;
    if (K > 0) P = P + h_above * A.gH;
    if (K < nk) h_above = A.h[n2 + hpl * K];
    double rT, rS;
    eos_density_derivs(A.E, v[0], v[1], (A.ref_pres >= 0.) ? A.ref_pres : P, rT, rS);
    double *r = A.irec;
    r[irec_at(K, n2, 0, hpl, nk)] = P; r[irec_at(K, n2, 1, hpl, nk)] = v[0]; r[irec_at(K, n2, 2, hpl, nk)] = v[1];
    r[irec_at(K, n2, 3, hpl, nk)] = rT; r[irec_at(K, n2, 4, hpl, nk)] = rS;
  });
}

// find_neutral_surface_positions_continuous :1353 (KoL / KoR keep the reference's 1-based layer numbers)
template <int DIR>
__global__ __launch_bounds__(64) void nd_surfaces_kernel(NDArgs A, int nbx) {
  const m6::GridDev &g = A.g;
  const NDFace F = nd_face<DIR>(g, nbx);
  if (!F.has) return;
  const long f = F.f, pl = F.pl, hpl = F.hpl, cl = F.cl, cr = F.cr;
  if (!F.wet) { nd_dry_surfaces<DIR>(A, f, pl); return; }
  double *__restrict__ PoL = A.PoL[DIR], *__restrict__ PoR = A.PoR[DIR], *__restrict__ hEff = A.hEff[DIR];
  ko_t *__restrict__ KoL = A.KoL[DIR], *__restrict__ KoR = A.KoR[DIR];
  const int ns = A.ns, nk = g.nk;
  const double *__restrict__ irec = A.irec;
  // The walk reads interface klm1 = max(kl-1, 1), klm1+1 and kl of the left column (and the same of the right): two interfaces a side
  // are kept in registers -- A at klm1, B at klm1+1; interface kl is A while kl = 1 and B afterwards -- and a step that moves kl or kr
  // down by one loads one new interface: one record (the lanes of a wave stand at different depths, so every load here is a gather).
  struct Iface { double P, T, S, rT, rS; };
  auto load = [&](long c, int k) {
    return Iface{irec[irec_at(k - 1, c, 0, hpl, nk)], irec[irec_at(k - 1, c, 1, hpl, nk)], irec[irec_at(k - 1, c, 2, hpl, nk)],
                 irec[irec_at(k - 1, c, 3, hpl, nk)], irec[irec_at(k - 1, c, 4, hpl, nk)]};
  };
  auto loadL = [&](int k) { return load(cl, k); };
  auto loadR = [&](int k) { return load(cr, k); };
  auto PL = [&](int k) { return irec[irec_at(k - 1, cl, 0, hpl, nk)]; };
  auto PR = [&](int k) { return irec[irec_at(k - 1, cr, 0, hpl, nk)]; };
  Iface LA = loadL(1), LB = loadL(2), RA = loadR(1), RB = loadR(2);
  const int bl_kl = A.interior ? A.kbot[cl] : 0, bl_kr = A.interior ? A.kbot[cr] : 0;      // :1508-1521 (no layer number is <= 0)
  const double bl_zl = A.interior ? A.zbot[cl] : 0., bl_zr = A.interior ? A.zbot[cr] : 0.;
  int kr = 1, kl = 1, lastK_right = 1, lastK_left = 1;
  double lastP_right = 0., lastP_left = 0., absL_prev = 0., absR_prev = 0.;
  bool reached_bottom = false, searching_left = false, searching_right = false;
  for (int ks = 0; ks < ns; ks++) {
    int klm1 = (kl - 1 > 1) ? kl - 1 : 1;
    int krm1 = (kr - 1 > 1) ? kr - 1 : 1;
    const Iface Lk = (kl == 1) ? LA : LB, Rk = (kr == 1) ? RA : RB;
    const double Tr_kr = Rk.T, Sr_kr = Rk.S, aTr_kr = Rk.rT, aSr_kr = Rk.rS;
    const double Tl_kl = Lk.T, Sl_kl = Lk.S, aTl_kl = Lk.rT, aSl_kl = Lk.rS;
    const double dRho = 0.5 * ((aTr_kr + aTl_kl) * (Tr_kr - Tl_kl) + (aSr_kr + aSl_kl) * (Sr_kr - Sl_kl));
    if (!reached_bottom) {
      if (dRho < 0.) { searching_left = true; searching_right = false; }
      else if (dRho > 0.) { searching_right = true; searching_left = false; }
      else if (kl + kr == 2) { searching_left = true; searching_right = false; }
      else { searching_left = !searching_left; searching_right = !searching_right; }
    }
    double pL, pR;
    int oKL, oKR;
    if (searching_left) {
      const double dRhoTop = 0.5 * ((LA.rT + aTr_kr) * (LA.T - Tr_kr) + (LA.rS + aSr_kr) * (LA.S - Sr_kr));
      const double dRhoBot = 0.5 * ((LB.rT + aTr_kr) * (LB.T - Tr_kr) + (LB.rS + aSr_kr) * (LB.S - Sr_kr));
      if (dRhoTop > 0. || kr + kl == 2) pL = 0.;
      else if (dRhoTop >= dRhoBot) pL = 1.;
      else pL = interp_nondim(dRhoTop, LA.P, dRhoBot, LB.P);
      if (pL >= 1. && klm1 < nk) { klm1 = klm1 + 1; pL = pL - 1.; }
      if ((double)(klm1 - lastK_left) + (pL - lastP_left) < 0.) { pL = lastP_left; klm1 = lastK_left; }
      oKL = klm1;
      if (kr <= nk) { pR = 0.; oKR = kr; } else { pR = 1.; oKR = nk; }
      if (kr <= nk) {
        kr = kr + 1;
        if (kr > 2) { RA = RB; RB = loadR(kr); }
      } else { reached_bottom = true; searching_right = true; searching_left = false; }
    } else {
      const double dRhoTop = 0.5 * ((RA.rT + aTl_kl) * (RA.T - Tl_kl) + (RA.rS + aSl_kl) * (RA.S - Sl_kl));
      const double dRhoBot = 0.5 * ((RB.rT + aTl_kl) * (RB.T - Tl_kl) + (RB.rS + aSl_kl) * (RB.S - Sl_kl));
      if (dRhoTop >= 0. || kr + kl == 2) pR = 0.;
      else if (dRhoTop >= dRhoBot) pR = 1.;
      else pR = interp_nondim(dRhoTop, RA.P, dRhoBot, RB.P);
      if (pR >= 1. && krm1 < nk) { krm1 = krm1 + 1; pR = pR - 1.; }
      if ((double)(krm1 - lastK_right) + (pR - lastP_right) < 0.) { pR = lastP_right; krm1 = lastK_right; }
      oKR = krm1;
      if (kl <= nk) { pL = 0.; oKL = kl; } else { pL = 1.; oKL = nk; }
      if (kl <= nk) {
        kl = kl + 1;
        if (kl > 2) { LA = LB; LB = loadL(kl); }
      } else { reached_bottom = true; searching_right = false; searching_left = true; }
    }
    if (oKL <= bl_kl) { oKL = bl_kl; if (pL < bl_zl) pL = bl_zl; }
    if (oKR <= bl_kr) { oKR = bl_kr; if (pR < bl_zr) pR = bl_zr; }
    PoL[f + pl * ks] = pL; PoR[f + pl * ks] = pR; KoL[f + pl * ks] = (ko_t)oKL; KoR[f + pl * ks] = (ko_t)oKR;
    lastK_left = oKL; lastP_left = pL; lastK_right = oKR; lastP_right = pR;
    // absolute_position :2258 of this surface; that of the one above is the value formed a step ago from the same expression
    const double PL0 = PL(oKL), PR0 = PR(oKR);
    const double absL = PL0 + pL * (PL(oKL + 1) - PL0), absR = PR0 + pR * (PR(oKR + 1) - PR0);
    if (ks > 0) {
      const double hL = absL - absL_prev, hR = absR - absR_prev;
      double he = 0.;
      if (hL + hR > 0.) he = 2. * hL * hR / (hL + hR);
      hEff[f + pl * (ks - 1)] = he * A.pa_to_H;      // :570-575
    }
    absL_prev = absL; absR_prev = absR;
  }
}

// compute_tapering_coeffs :1044-1058 for one wet face: k_min and k_max of the left and of the right column
template <int DIR>
__global__ __launch_bounds__(64) void nd_taper_kernel(NDArgs A, int nbx) {
  const m6::GridDev &g = A.g;
  const NDFace F = nd_face<DIR>(g, nbx);
  if (!F.wet) return;      // (read by the wet faces only)
  const long f = F.f, pl = F.pl, hpl = F.hpl, cl = F.cl, cr = F.cr;
  const int nk = g.nk;
  const double bld_l = A.hbl[cl], bld_r = A.hbl[cr];
  const double max_bld = max2(bld_l, bld_r), min_bld = min2(bld_l, bld_r);
  int k[4];
  double zeta;
  boundary_k_range_surface(A.h + cl, hpl, nk, min_bld, k[0], zeta);
  boundary_k_range_surface(A.h + cl, hpl, nk, max_bld, k[1], zeta);
  boundary_k_range_surface(A.h + cr, hpl, nk, min_bld, k[2], zeta);
  boundary_k_range_surface(A.h + cr, hpl, nk, max_bld, k[3], zeta);
#pragma unroll
  for (int q = 0; q < 4; q++) A.kt[DIR][f + pl * q] = (ko_t)k[q];
}

// coeff_l(K) / coeff_r(K) :1059-1073 of the interface K (1-based) from k_min and k_max of the column
__device__ __forceinline__ double taper_coeff(int K, int k_min, int k_max) {
  if (K <= k_min) return 0.0;
  if (K <= k_max + 1) return ((double)(K - k_min) + 1.0) / ((double)(k_max - k_min) + 2.0);
  return 1.0;
}

// Coef_h :670-684 of a wet column of the compute domain; Coef_x(I,j,K), Coef_y(i,J,K) as MOM_tracer_hor_diff.F90:489-518 forms them
__global__ __launch_bounds__(64) void nd_coef_h_kernel(NDArgs A) {
  const m6::GridDev &g = A.g;
  const int i = g.isc + blockIdx.x * 64 + threadIdx.x, j = g.jsc + blockIdx.y, nk = g.nk;
  if (i > g.iec) return;
  const long n2 = g.h2(i, j), hpl = (long)g.nih * g.njh;
  if (!(g.mask2dT[n2] > 0.)) return;
  const int I = i, J = j;
  const long uW = g.u2(I - 1, j), uE = g.u2(I, j), vS = g.v2(i, J - 1), vN = g.v2(i, J);
  const long nW = g.h2(i - 1, j), nE = g.h2(i + 1, j), nS = g.h2(i, j - 1), nN = g.h2(i, j + 1);
  const double normalize = 1.0 / ((g.mask2dCu[uW] + g.mask2dCu[uE]) + (g.mask2dCv[vS] + g.mask2dCv[vN]) + 1.0e-37);
  const double nm = normalize * g.mask2dT[n2];
  const double cW = A.scale * A.khdt[0][uW], cE = A.scale * A.khdt[0][uE], cS = A.scale * A.khdt[1][vS], cN = A.scale * A.khdt[1][vN];
  const double *__restrict__ ebt = A.ebt;
  double *__restrict__ coef_h = A.coef_h;
  coef_h[n2] = nm * ((cW + cE) + (cS + cN));
  for (int K = 1; K <= nk; K++) {
    const long o = hpl * (K - 1);
    const double e = ebt[n2 + o];
    const double xW = cW * 0.5 * (ebt[nW + o] + e), xE = cE * 0.5 * (e + ebt[nE + o]);
    const double yS = cS * 0.5 * (ebt[nS + o] + e), yN = cN * 0.5 * (e + ebt[nN + o]);
    coef_h[n2 + hpl * K] = nm * ((xW + xE) + (yS + yN));
  }
}

// the interface values of the batch's tracers (neutral_surface_flux :2373-2374) and the means of their cells, as records
__global__ __launch_bounds__(64) void nd_tracer_cols_kernel(NDArgs A, int nbx) {
  const m6::GridDev &g = A.g;
  const NDCol C = nd_column(g, nbx);
  if (!C.has) return;
  const long n2 = C.n2, hpl = C.hpl;
  const int nk = g.nk;
  const double *ts[ND_BATCH];
#pragma unroll
  for (int z = 0; z < ND_BATCH; z++) ts[z] = A.t[z < A.nb ? z : 0];
  walk_interfaces<ND_BATCH>(A.h, ts, A.nb, n2, hpl, nk, A.h_neglect, [&](int K, const double *v, const double *m) {
    double2 *r = (double2 *)(A.trec + ((long)K * hpl + n2) * TREC);
    r[0] = make_double2(v[0], v[1]); r[1] = make_double2(v[2], v[3]);
    r[2] = make_double2(m[0], m[1]); r[3] = make_double2(m[2], m[3]);
  });
}

// neutral_surface_flux :2297 (continuous).  SYM: the tendencies of the two cells of the face from its fluxes, layer by layer (the order
// of the sums of neutral_diffusion :939-954: a face at a time, its surfaces top down); otherwise the fluxes.  COEF: what coeff_l / coeff_r
// are -- absent (khtr_ave = 1), the taper, Coef_h, or their product (:703-764); with Coef_h the fluxes carry the diffusivity (:834-878)
// D: nothing, or (the symmetric order) one NDTransOut -- the form that also leaves trans_x_2d / trans_y_2d (:935-989) of the batch
enum { ND_COEF_NONE = 0, ND_COEF_TAPER = 1, ND_COEF_EBT = 2, ND_COEF_BOTH = 3 };
template <int DIR, bool SYM, int COEF = ND_COEF_NONE, typename... D>
__global__ __launch_bounds__(64) void nd_flux_kernel(NDArgs A, int nbx, D... d) {
  constexpr bool DIAG = sizeof...(D) > 0;
  static_assert(!DIAG || SYM, "the order of 2024 and before keeps the fluxes: nd_trans_march_kernel sums them");
  const m6::GridDev &g = A.g;
  const NDFace F = nd_face<DIR>(g, nbx);
  if (!F.has) return;
  const long f = F.f, pl = F.pl, hpl = F.hpl, cl = F.cl, cr = F.cr;
  double *__restrict__ Flx = A.Flx[DIR];
  double *__restrict__ tdL = A.tend[DIR][0], *__restrict__ tdR = A.tend[DIR][1];
  const int ns = A.ns, nb = A.nb, nk = g.nk;
  if (!F.wet) {
    for (int z = 0; z < nb; z++) nd_dry_fluxes<SYM>(ns, nk, Flx, tdL, tdR, A.flx_stride * z + f, pl);
    if constexpr (DIAG) {
      const NDTransOut &T = nd_first(d...);
      for (int z = 0; z < nb; z++) if (T.trans[z]) T.trans[z][f] = 0.;
    }
    return;
  }
  const double *__restrict__ PiL = A.PoL[DIR], *__restrict__ PiR = A.PoR[DIR], *__restrict__ hEff = A.hEff[DIR];
  const ko_t *__restrict__ KoL = A.KoL[DIR], *__restrict__ KoR = A.KoR[DIR];
  const double cf = A.scale * A.khdt[DIR][f];
  int bad = 0;
  double pLt = PiL[f], pRt = PiR[f];
  int klt = KoL[f] - 1, krt = KoR[f] - 1;
  // A side of the face: the cell the surface is in, with the records of the interfaces above and below it (the interface values i0, i1 of
  // the batch's tracers, the means m0 of the cell and m1 of the cell below), the limited edge values of the cell
  // (ppm_left_right_edge_values :2541) and the value at the surface above (the reference's T_*_top of a sublayer is its T_*_bottom of the
  // sublayer above: the same expression of the same numbers).  A surface that enters the next cell needs one new record.
  struct Side { double i0[ND_BATCH], i1[ND_BATCH], m0[ND_BATCH], m1[ND_BATCH], eL[ND_BATCH], eR[ND_BATCH], top[ND_BATCH]; };
  auto load = [&](long c, int K, double *iv, double *mv) {
    const double2 *r = (const double2 *)(A.trec + ((long)K * hpl + c) * TREC);
    const double2 a = r[0], b = r[1], c2 = r[2], d = r[3];
    iv[0] = a.x; iv[1] = a.y; iv[2] = b.x; iv[3] = b.y; mv[0] = c2.x; mv[1] = c2.y; mv[2] = d.x; mv[3] = d.y;
  };
  auto enter = [&](Side &s, long c, int k_old, int k_new) {      // the records of the cell k_new
    if (k_new == k_old + 1) {
#pragma unroll
      for (int z = 0; z < ND_BATCH; z++) { s.i0[z] = s.i1[z]; s.m0[z] = s.m1[z]; }
    } else {
      load(c, k_new, s.i0, s.m0);
    }
    load(c, k_new + 1, s.i1, s.m1);
  };
  Side sl, sr;
  load(cl, klt, sl.i0, sl.m0); load(cl, klt + 1, sl.i1, sl.m1);
  load(cr, krt, sr.i0, sr.m0); load(cr, krt + 1, sr.i1, sr.m1);
#pragma unroll
  for (int z = 0; z < ND_BATCH; z++) {
    sl.top[z] = (1. - pLt) * sl.i0[z] + pLt * sl.i1[z];
    sr.top[z] = (1. - pRt) * sr.i0[z] + pRt * sr.i1[z];
    ppm_edges(sl.i0[z], sl.i1[z], sl.m0[z], sl.eL[z], sl.eR[z]);
    ppm_edges(sr.i0[z], sr.i1[z], sr.m0[z], sr.eL[z], sr.eR[z]);
  }
  // SYM: the running sums of the layers klt, krt; every layer of the two columns is stored once (zero where no sublayer lies in it)
  double accL[ND_BATCH], accR[ND_BATCH];
#pragma unroll
  for (int z = 0; z < ND_BATCH; z++) { accL[z] = 0.; accR[z] = 0.; }
  [[maybe_unused]] double trn[DIAG ? ND_BATCH : 1];      // DIAG: trans_x_2d(I,j) | trans_y_2d(i,J) of the batch's tracers
  if constexpr (DIAG) {
#pragma unroll
    for (int z = 0; z < ND_BATCH; z++) trn[z] = 0.;
  }
  // COEF: coeff_l / coeff_r at the interface K (0-based: the top of the cell K), and their values at the surface above
  int kminL = 0, kmaxL = 0, kminR = 0, kmaxR = 0;
  if constexpr ((COEF & ND_COEF_TAPER) != 0) {
    const ko_t *__restrict__ kt = A.kt[DIR];
    kminL = kt[f]; kmaxL = kt[f + pl]; kminR = kt[f + pl * 2]; kmaxR = kt[f + pl * 3];
  }
  auto coefL = [&](int K) -> double {
    if constexpr (COEF == ND_COEF_TAPER) return taper_coeff(K + 1, kminL, kmaxL);
    else if constexpr (COEF == ND_COEF_EBT) return A.coef_h[cl + hpl * K];
    else return taper_coeff(K + 1, kminL, kmaxL) * A.coef_h[cl + hpl * K];
  };
  auto coefR = [&](int K) -> double {
    if constexpr (COEF == ND_COEF_TAPER) return taper_coeff(K + 1, kminR, kmaxR);
    else if constexpr (COEF == ND_COEF_EBT) return A.coef_h[cr + hpl * K];
    else return taper_coeff(K + 1, kminR, kmaxR) * A.coef_h[cr + hpl * K];
  };
  double cLt = 0., cRt = 0.;
  if constexpr (COEF != ND_COEF_NONE) { cLt = coefL(klt); cRt = coefR(krt); }
  if (SYM) {
    for (int z = 0; z < nb; z++) {
      nd_tend_store(tdL, A.flx_stride * z + f, pl, -1, klt, 0.);
      nd_tend_store(tdR, A.flx_stride * z + f, pl, -1, krt, 0.);
    }
  }
  for (int ks = 0; ks < ns - 1; ks++) {
    const double pLb = PiL[f + pl * (ks + 1)], pRb = PiR[f + pl * (ks + 1)];
    const int klb = KoL[f + pl * (ks + 1)] - 1, krb = KoR[f + pl * (ks + 1)] - 1;
    const double he = hEff[f + pl * ks];
    if (klb < klt || krb < krt) bad |= 2;      // (the positions of the surfaces never move up a column)
    double lay_l[ND_BATCH], lay_r[ND_BATCH];   // the means of the sublayer in the cells klt, krt
    if (he != 0.) {
#pragma unroll
      for (int z = 0; z < ND_BATCH; z++) {
        lay_l[z] = ppm_ave(pLt, pLb + (double)(klb - klt), sl.eL[z], sl.eR[z], sl.m0[z], bad);
        lay_r[z] = ppm_ave(pRt, pRb + (double)(krb - krt), sr.eL[z], sr.eR[z], sr.m0[z], bad);
      }
    }
    if (klb != klt) enter(sl, cl, klt, klb);
    if (krb != krt) enter(sr, cr, krt, krb);
    double khtr_ave = 1.0;
    if constexpr (COEF != ND_COEF_NONE) {      // :2410-2417
      const double cLb = (klb != klt) ? coefL(klb) : cLt, cRb = (krb != krt) ? coefR(krb) : cRt;
      khtr_ave = 0.25 * ((cLb + cLt) + (cRb + cRt));
      cLt = cLb; cRt = cRb;
    }
#pragma unroll
    for (int z = 0; z < ND_BATCH; z++) {
      const double T_left_bottom = (1. - pLb) * sl.i0[z] + pLb * sl.i1[z];
      const double T_right_bottom = (1. - pRb) * sr.i0[z] + pRb * sr.i1[z];
      double flx = 0.;
      if (he != 0.) {
        const double T_left_top = sl.top[z], T_right_top = sr.top[z];
        const double T_left_layer = lay_l[z], T_right_layer = lay_r[z];
        const double dT_top = T_right_top - T_left_top;
        const double dT_bottom = T_right_bottom - T_left_bottom;
        double dT_ave = 0.5 * (dT_top + dT_bottom);
        const double dT_layer = T_right_layer - T_left_layer;
        if (signum(1., dT_top) * signum(1., dT_bottom) <= 0. || signum(1., dT_ave) * signum(1., dT_layer) <= 0.) dT_ave = 0.;
        else dT_ave = dT_layer;
        flx = dT_ave * he * khtr_ave;
      }
      if (SYM && (COEF & ND_COEF_EBT) != 0) { accL[z] = accL[z] + flx; accR[z] = accR[z] - flx; }
      else if (SYM) { accL[z] = accL[z] + cf * flx; accR[z] = accR[z] - cf * flx; }
      else if (z < nb) Flx[A.flx_stride * z + f + pl * ks] = flx;
      if constexpr (DIAG) {
        if ((COEF & ND_COEF_EBT) != 0) trn[z] = trn[z] - flx;
        else trn[z] = trn[z] - cf * flx;
      }
      sl.top[z] = T_left_bottom; sr.top[z] = T_right_bottom;
    }
    // the surface enters another cell: its edge values from the interface values and the mean just read; SYM: the layer it leaves is done
    if (klb != klt) {
#pragma unroll
      for (int z = 0; z < ND_BATCH; z++) {
        ppm_edges(sl.i0[z], sl.i1[z], sl.m0[z], sl.eL[z], sl.eR[z]);
        if (SYM) {
          if (z < nb) nd_tend_store(tdL, A.flx_stride * z + f, pl, klt, klb, accL[z]);
          accL[z] = 0.;
        }
      }
    }
    if (krb != krt) {
#pragma unroll
      for (int z = 0; z < ND_BATCH; z++) {
        ppm_edges(sr.i0[z], sr.i1[z], sr.m0[z], sr.eL[z], sr.eR[z]);
        if (SYM) {
          if (z < nb) nd_tend_store(tdR, A.flx_stride * z + f, pl, krt, krb, accR[z]);
          accR[z] = 0.;
        }
      }
    }
    pLt = pLb; pRt = pRb; klt = klb; krt = krb;
  }
  if (SYM) {
    for (int z = 0; z < nb; z++) {
      nd_tend_store(tdL, A.flx_stride * z + f, pl, klt, nk, accL[z]);
      nd_tend_store(tdR, A.flx_stride * z + f, pl, krt, nk, accR[z]);
    }
  }
  if constexpr (DIAG) {
    const NDTransOut &T = nd_first(d...);
#pragma unroll
    for (int z = 0; z < ND_BATCH; z++) if (z < nb && T.trans[z]) T.trans[z][f] = trn[z] * T.Idt;
  }
  if (bad) atomicOr(A.bad, bad);
}

// trans_x_2d / trans_y_2d (:935-989) in the order of 2024 and before, where the fluxes of the batch stand in scratch: one thread a face
// marches the surfaces, trans = trans - Coef(:,:,1)*Flx(ks) with Coef as nd_update_kernel<false> forms it, or trans - Flx(ks) where the
// fluxes carry the coefficient (EBT); dry faces get 0
template <int DIR, bool EBT>
__global__ __launch_bounds__(64) void nd_trans_march_kernel(NDFaces A, int nbx, NDTransOut T) {
  const m6::GridDev &g = A.g;
  const NDFace F = nd_face<DIR>(g, nbx);
  if (!F.has) return;
  const long f = F.f, pl = F.pl;
  const double cf = A.scale * A.khdt[DIR][f];
  for (int z = 0; z < A.nb; z++) {
    if (!T.trans[z]) continue;
    double trans = 0.;
    if (F.wet) {
      const double *__restrict__ Flx = A.Flx[DIR] + A.flx_stride * z + f;
      for (int ks = 0; ks < A.ns - 1; ks++) trans = EBT ? trans - Flx[pl * ks] : trans - cf * Flx[pl * ks];
      trans = trans * T.Idt;
    }
    T.trans[z][f] = trans;
  }
}

// :955-959 after the sums of :939-954 (the symmetric order): the four faces' tendencies of the layer, then the tracer
// D: nothing, or one NDMixOut -- the form that also stores the tendency (:871-875, :916-920) and its concentration form (:1010-1014)
template <typename... D>
__global__ __launch_bounds__(256) void nd_update_sym_kernel(NDFaces A, D... d) {
  constexpr bool DIAG = sizeof...(D) > 0;
  const m6::GridDev &g = A.g;
  const int i = g.isc + blockIdx.x * 256 + threadIdx.x, j = g.jsc + blockIdx.y, k = blockIdx.z % g.nk, z = blockIdx.z / g.nk;
  if (i > g.iec) return;
  const long n2 = g.h2(i, j), hpl = (long)g.nih * g.njh;
  if (!(g.mask2dT[n2] > 0.)) {
    if constexpr (DIAG) {      // tendency(:,:,:) = 0. (:696)
      const NDMixOut &M = nd_first(d...);
      if (M.cont[z]) M.cont[z][n2 + hpl * k] = 0.;
      if (M.conc[z]) M.conc[z][n2 + hpl * k] = 0.;
    }
    return;
  }
  const long upl = (long)(g.nih + 1) * g.njh, vpl = (long)g.nih * (g.njh + 1);
  const double tN = A.tend[1][0][A.flx_stride * z + g.v2(i, j) + vpl * k], tS = A.tend[1][1][A.flx_stride * z + g.v2(i, j - 1) + vpl * k];
  const double tE = A.tend[0][0][A.flx_stride * z + g.u2(i, j) + upl * k], tW = A.tend[0][1][A.flx_stride * z + g.u2(i - 1, j) + upl * k];
  const double tendency = (tN + tS) + (tE + tW);
  double *__restrict__ t = A.t[z];
  double x = t[n2 + hpl * k] + tendency * (g.IareaT[n2] / (A.h[n2 + hpl * k] + g.H_subroundoff));
  if (fabs(x) < A.cu[z]) x = 0.0;
  t[n2 + hpl * k] = x;
  if constexpr (DIAG) {
    const NDMixOut &M = nd_first(d...);
    const double td = (tendency * g.IareaT[n2]) * M.Idt;
    if (M.cont[z]) M.cont[z][n2 + hpl * k] = td;
    if (M.conc[z]) M.conc[z][n2 + hpl * k] = td / (A.h[n2 + hpl * k] + g.H_subroundoff);
  }
}

// :921-938, :955-959 (the order of 2024 and before): the cell's tendency from the fluxes of its four faces, surface by surface round the
// faces E, W, N, S, accumulated per layer in LDS (the layer index is data: KoL / KoR), then the tracer.  (A thread per layer that walks
// the runs of its four faces -- no LDS, full occupancy -- reads the fluxes as gathers and is slower: profiles/r04_experiments.txt.)
// EBT: the fluxes carry the diffusivity (:834-848); otherwise they are multiplied by Coef_x(I,j,1), Coef_y(i,J,1) (:880-893)
// D: as nd_update_sym_kernel takes it
template <bool EBT, typename... D>
__global__ __launch_bounds__(64) void nd_update_kernel(NDFaces A, D... d) {
  constexpr bool DIAG = sizeof...(D) > 0;
  extern __shared__ double acc[];      // [nk][64]
  const m6::GridDev &g = A.g;
  const int lane = threadIdx.x, i = g.isc + blockIdx.x * 64 + lane, j = g.jsc + blockIdx.y, nk = g.nk, z = blockIdx.z;
  if (i > g.iec) return;
  const long n2 = g.h2(i, j), hpl = (long)g.nih * g.njh;
  if (!(g.mask2dT[n2] > 0.)) {
    if constexpr (DIAG) {      // tendency(:,:,:) = 0. (:696)
      const NDMixOut &M = nd_first(d...);
      for (int k = 0; k < nk; k++) {
        if (M.cont[z]) M.cont[z][n2 + hpl * k] = 0.;
        if (M.conc[z]) M.conc[z][n2 + hpl * k] = 0.;
      }
    }
    return;
  }
  double *__restrict__ t = A.t[z];
  const long upl = (long)(g.nih + 1) * g.njh, vpl = (long)g.nih * (g.njh + 1);
  const long uE = g.u2(i, j), uW = g.u2(i - 1, j), vN = g.v2(i, j), vS = g.v2(i, j - 1);
  const double cE = A.scale * A.khdt[0][uE], cW = A.scale * A.khdt[0][uW], cN = A.scale * A.khdt[1][vN], cS = A.scale * A.khdt[1][vS];
  const int ns = A.ns;
  const ko_t *__restrict__ uKoL = A.KoL[0], *__restrict__ uKoR = A.KoR[0], *__restrict__ vKoL = A.KoL[1], *__restrict__ vKoR = A.KoR[1];
  const double *__restrict__ uFlx = A.Flx[0] + A.flx_stride * z, *__restrict__ vFlx = A.Flx[1] + A.flx_stride * z;
#define ACC(k) acc[(k) * 64 + lane]
  // The surfaces are taken eight at a time: the loads of a group (layer numbers and fluxes of the four faces) are issued together, then
  // the group's contributions are added in the reference's order.
  constexpr int NU = 8;
  const int nl = ns - 1;
  for (int k = 0; k < nk; k++) ACC(k) = 0.;
  for (int ks0 = 0; ks0 < nl; ks0 += NU) {
    int kE[NU], kW[NU], kN[NU], kS[NU];
    double fE[NU], fW[NU], fN[NU], fS[NU];
#pragma unroll
    for (int q = 0; q < NU; q++) {
      const int ks = (ks0 + q < nl) ? ks0 + q : nl - 1;
      kE[q] = uKoL[uE + upl * ks] - 1; fE[q] = uFlx[uE + upl * ks];
      kW[q] = uKoR[uW + upl * ks] - 1; fW[q] = uFlx[uW + upl * ks];
      kN[q] = vKoL[vN + vpl * ks] - 1; fN[q] = vFlx[vN + vpl * ks];
      kS[q] = vKoR[vS + vpl * ks] - 1; fS[q] = vFlx[vS + vpl * ks];
    }
#pragma unroll
    for (int q = 0; q < NU; q++) {
      if (ks0 + q < nl) {
        if (EBT) {
          ACC(kE[q]) = ACC(kE[q]) + fE[q];
          ACC(kW[q]) = ACC(kW[q]) - fW[q];
          ACC(kN[q]) = ACC(kN[q]) + fN[q];
          ACC(kS[q]) = ACC(kS[q]) - fS[q];
        } else {
          ACC(kE[q]) = ACC(kE[q]) + cE * fE[q];
          ACC(kW[q]) = ACC(kW[q]) - cW * fW[q];
          ACC(kN[q]) = ACC(kN[q]) + cN * fN[q];
          ACC(kS[q]) = ACC(kS[q]) - cS * fS[q];
        }
      }
    }
  }
  const double IareaT = g.IareaT[n2];
  for (int k = 0; k < nk; k++) {
    double x = t[n2 + hpl * k] + ACC(k) * (IareaT / (A.h[n2 + hpl * k] + g.H_subroundoff));
    if (fabs(x) < A.cu[z]) x = 0.0;
    t[n2 + hpl * k] = x;
    if constexpr (DIAG) {
      const NDMixOut &M = nd_first(d...);
      const double td = (ACC(k) * IareaT) * M.Idt;
      if (M.cont[z]) M.cont[z][n2 + hpl * k] = td;
      if (M.conc[z]) M.conc[z][n2 + hpl * k] = td / (A.h[n2 + hpl * k] + g.H_subroundoff);
    }
  }
#undef ACC
}

}  // namespace

namespace m6 {

int neutral_drive(const HordiffCall &c, const mom6hip_neutral_diffusion_cs_t *nd, NDFaces &S, const NDBranch &b) {
  mom6hip_ctx_t *ctx = c.ctx;
  const std::vector<double *> &d_tr = c.d_tr;
  const int ntr = (int)d_tr.size();
  M6_REQUIRE(c.idx_T >= 0 && c.idx_T < ntr && c.idx_S >= 0 && c.idx_S < ntr, "tracer_hordiff: tv%%T and tv%%S must be among the tracers (idx_T, idx_S)");
  const m6::GridDev g = ctx->g;
  M6_REQUIRE(g.mask2dT && g.mask2dCu && g.mask2dCv && g.IareaT, "neutral_diffusion: mask2dT, mask2dCu, mask2dCv and IareaT are needed");
  M6_REQUIRE(g.nk >= 2 && g.nk <= 128, "neutral_diffusion: 2 to 128 layers are supported");
  hipStream_t s = ctx->stream;
  const int nk = g.nk, ns = b.ns;
  const size_t hpl = (size_t)g.nih * g.njh, upl = (size_t)(g.nih + 1) * g.njh, vpl = (size_t)g.nih * (g.njh + 1);
  const size_t fpl = upl > vpl ? upl : vpl;
  const bool symmetric = nd->ndiff_answer_date > 20240330, interior = nd->interior_only != 0;
  S.g = g; S.h = c.h; S.scale = c.I_numitts; S.ns = ns; S.khdt[0] = c.khdt_x; S.khdt[1] = c.khdt_y;
  const int nbmax = ntr < ND_BATCH ? ntr : ND_BATCH;
  // per direction PoL, PoR, hEff [surface][faces]; then per tracer of a batch either the fluxes [surface][faces] of the two directions or
  // the tendencies [layer][faces] of the two sides of the faces of the two directions
  const size_t per_tracer = symmetric ? fpl * nk * 4 : fpl * ns * 2;
  double *faces = (double *)c.st.scratch(sizeof(double) * (fpl * ns * 6 + per_tracer * (size_t)nbmax));
  ko_t *kos = (ko_t *)c.st.scratch(sizeof(ko_t) * fpl * ns * 4);
  int *bad = (int *)c.st.scratch(64);
  double *hbl = nullptr;
  if (interior) {      // :370-390: CS%hbl = visc%h_ML, pass_var(CS%hbl, halo=1)
    M6_REQUIRE(c.h_ML != nullptr, "hor_bnd_diffusion requires that visc%%h_ML is associated.");
    hbl = (double *)c.st.scratch(sizeof(double) * hpl);
    M6_REQUIRE(!c.st.failed() && hbl, "neutral_diffusion: out of device memory");
  }
  if (int rc = b.scratch(hbl)) return rc;
  M6_REQUIRE(!c.st.failed() && faces && kos && bad, "neutral_diffusion: out of device memory");
  S.bad = bad;
  double *per = faces + fpl * ns * 6;
  for (int d = 0; d < 2; d++) {
    S.PoL[d] = faces + fpl * ns * (3 * d); S.PoR[d] = S.PoL[d] + fpl * ns; S.hEff[d] = S.PoR[d] + fpl * ns;
    S.KoL[d] = kos + fpl * ns * (2 * d); S.KoR[d] = S.KoL[d] + fpl * ns;
    S.Flx[d] = symmetric ? nullptr : per + fpl * ns * d;
    S.tend[d][0] = symmetric ? per + fpl * nk * (2 * d) : nullptr; S.tend[d][1] = symmetric ? per + fpl * nk * (2 * d + 1) : nullptr;
  }
  S.flx_stride = (long)per_tracer;
  M6_HIP(hipMemsetAsync(bad, 0, sizeof(int), s));
  // the diagnostics neutral_diffusion posts (:935-1014): where only dfxy_cont_2d is asked for, the tendency of a batch goes to scratch
  const MixDiag *mix = c.mix;
  bool any_mix = false, cont_to_scratch = false;
  if (mix) for (int m = 0; m < ntr; m++) {
    for (int q = MIX_DFX_2D; q <= MIX_DFXY_CONC; q++) any_mix = any_mix || mix[m].a[q];
    cont_to_scratch = cont_to_scratch || (mix[m].a[MIX_DFXY_CONT_2D] && !mix[m].a[MIX_DFXY_CONT]);
  }
  double *cont_scr = nullptr;
  if (cont_to_scratch) {
    cont_scr = (double *)c.st.scratch(sizeof(double) * hpl * nk * (size_t)nbmax);
    M6_REQUIRE(!c.st.failed() && cont_scr, "neutral_diffusion: out of device memory for the diagnostics");
  }

  const int ni = g.iec - g.isc + 1, nj = g.jec - g.jsc + 1;
  std::vector<double *> pf(d_tr);
  std::vector<int32_t> ppos(ntr, MOM6HIP_POS_H), pnk(ntr, nk);
  auto calc_coeffs = [&]() -> int {      // neutral_diffusion_calc_coeffs :337
    if (interior) {
      M6_HIP(hipMemcpyAsync(hbl, c.h_ML, sizeof(double) * hpl, hipMemcpyDeviceToDevice, s));
      double *f1[1] = {hbl}; int32_t p1[1] = {MOM6HIP_POS_H}, n1[1] = {1};
      if (int rc = m6::group_pass(ctx, f1, p1, n1, 1)) return rc;
    }
    return b.surfaces();
  };
  if (int rc = m6::group_pass(ctx, pf.data(), ppos.data(), pnk.data(), ntr)) return rc;      // do_group_pass(CS%pass_t) :478
  (*c.halo_updates)++;
  if (int rc = calc_coeffs()) return rc;
  if (b.once) { if (int rc = b.once()) return rc; }
  for (int itt = 1; itt <= c.num_itts; itt++) {
    if (itt > 1) {
      if (int rc = m6::group_pass(ctx, pf.data(), ppos.data(), pnk.data(), ntr)) return rc;
      (*c.halo_updates)++;
      if (nd->recalc_neutral_surf) { if (int rc = calc_coeffs()) return rc; }
    }
    for (int m0 = 0; m0 < ntr; m0 += nbmax) {      // neutral_diffusion :605: the tracers are independent of each other, a batch at a time
      S.nb = (ntr - m0 < nbmax) ? ntr - m0 : nbmax;
      for (int z = 0; z < ND_BATCH; z++) { S.t[z] = z < S.nb ? d_tr[m0 + z] : nullptr; S.cu[z] = z < S.nb ? c.cu[m0 + z] : 0.; }
      // what the batch asked for: the launches without diagnostics are taken where it asked for nothing
      NDTransOut tx = {}, ty = {};
      NDMixOut mo = {};
      CellSumMarch sum2d; sum2d.g = g; sum2d.n = 0;
      bool has_tx = false, has_ty = false, has_mo = false;
      tx.Idt = ty.Idt = mo.Idt = c.Idt;
      if (any_mix) for (int z = 0; z < S.nb; z++) {
        double *const *a = mix[m0 + z].a;
        tx.trans[z] = a[MIX_DFX_2D]; ty.trans[z] = a[MIX_DFY_2D]; mo.conc[z] = a[MIX_DFXY_CONC];
        mo.cont[z] = a[MIX_DFXY_CONT] ? a[MIX_DFXY_CONT] : a[MIX_DFXY_CONT_2D] ? cont_scr + hpl * nk * z : nullptr;
        if (a[MIX_DFXY_CONT_2D]) { sum2d.a3[sum2d.n] = mo.cont[z]; sum2d.a2[sum2d.n] = a[MIX_DFXY_CONT_2D]; sum2d.n++; }
        has_tx = has_tx || tx.trans[z]; has_ty = has_ty || ty.trans[z]; has_mo = has_mo || mo.cont[z] || mo.conc[z];
      }
      b.tracer_cols();
      b.fluxes(symmetric, symmetric && has_tx ? &tx : nullptr, symmetric && has_ty ? &ty : nullptr);
      if (!symmetric && (has_tx || has_ty)) {      // the fluxes stand in scratch until the next batch
        const int nbu = (ni + 1 + 63) / 64, nbv = (ni + 63) / 64;
        if (has_tx && b.flux_has_coef) hipLaunchKernelGGL((nd_trans_march_kernel<0, true>), dim3(nbu * nj), dim3(64), 0, s, S, nbu, tx);
        else if (has_tx) hipLaunchKernelGGL((nd_trans_march_kernel<0, false>), dim3(nbu * nj), dim3(64), 0, s, S, nbu, tx);
        if (has_ty && b.flux_has_coef) hipLaunchKernelGGL((nd_trans_march_kernel<1, true>), dim3(nbv * (nj + 1)), dim3(64), 0, s, S, nbv, ty);
        else if (has_ty) hipLaunchKernelGGL((nd_trans_march_kernel<1, false>), dim3(nbv * (nj + 1)), dim3(64), 0, s, S, nbv, ty);
      }
      const dim3 gsym((ni + 255) / 256, nj, nk * S.nb), gupd((ni + 63) / 64, nj, S.nb);
      const size_t lds = sizeof(double) * 64 * nk;
      if (has_mo) {
        if (symmetric) hipLaunchKernelGGL((nd_update_sym_kernel<NDMixOut>), gsym, dim3(256), 0, s, S, mo);
        else if (b.flux_has_coef) hipLaunchKernelGGL((nd_update_kernel<true, NDMixOut>), gupd, dim3(64), lds, s, S, mo);
        else hipLaunchKernelGGL((nd_update_kernel<false, NDMixOut>), gupd, dim3(64), lds, s, S, mo);
        if (sum2d.n) cell_sum_march(sum2d, s);
      }
      else if (symmetric) hipLaunchKernelGGL(nd_update_sym_kernel<>, gsym, dim3(256), 0, s, S);
      else if (b.flux_has_coef) hipLaunchKernelGGL(nd_update_kernel<true>, gupd, dim3(64), lds, s, S);
      else hipLaunchKernelGGL(nd_update_kernel<false>, gupd, dim3(64), lds, s, S);
    }
  }
  M6_HIP(hipGetLastError());
  int hbad = 0;
  M6_HIP(hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, s));
  M6_HIP(hipStreamSynchronize(s));
  for (const NDBranch::Bad &e : b.bad) M6_REQUIRE(!(hbad & e.bit), "%s", e.message);
  return 0;
}

// the neutral branch of tracer_hordiff (MOM_tracer_hor_diff.F90:474-534) with the continuous reconstruction; c.ebt_struct is
// VarMix%ebt_struct with KHTR_USE_EBT_STRUCT (tracer_hordiff has checked that nd->unsupported[3] says the same) and null without
int neutral_branch(const HordiffCall &c, const mom6hip_neutral_diffusion_cs_t *nd, const mom6hip_ndiff_discontinuous_cs_t *ndd) {
  static const char *names[8] = {"NDIFF_CONTINUOUS = False", "(free)", "NDIFF_TAPERING", "KHTR_USE_EBT_STRUCT",
                                 "NDIFF_USE_UNMASKED_TRANSPORT_BUG", "the neutral-diffusion diagnostics", "(free)", "(free)"};
  const mom6hip_eos_t *eos = c.eos;
  M6_REQUIRE(nd != nullptr && eos != nullptr, "tracer_hordiff: USE_NEUTRAL_DIFFUSION needs the neutral_diffusion control structure and tv%%eqn_of_state");
  M6_REQUIRE(nd->initialized, "neutral_diffusion: the control structure is not initialised");
  if (nd->unsupported[0] && ndd) {      // NDIFF_CONTINUOUS = False with its parameters: neutral_diffusion_disc.hip
    for (int q = 4; q < 8; q++) M6_REQUIRE((q == 5 && c.mix) || !nd->unsupported[q], "neutral_diffusion: %s is not provided by libmom6hip", names[q]);
    return neutral_disc_branch(c, nd, ndd);
  }
  // unsupported[2] (tapering) and [3] (KhTh_use_ebt_struct) are the switches of the two modes of the fluxes
  // ([5], the diagnostics, is taken with the records of mom6hip_tracer_hordiff_mix_diag: neutral_drive)
  for (int q = 0; q < 8; q++)
    M6_REQUIRE(q == 2 || q == 3 || (q == 5 && c.mix) || !nd->unsupported[q], "neutral_diffusion: %s is not provided by libmom6hip", names[q]);
  const bool taper = nd->unsupported[2] != 0, ebt = c.ebt_struct != nullptr;
  M6_REQUIRE(!taper || nd->interior_only, "neutral_diffusion: NDIFF_TAPERING is read with NDIFF_INTERIOR_ONLY only (the reference never reads it "
             "otherwise): it is refused without");
  const m6::GridDev g = c.ctx->g;
  hipStream_t s = c.ctx->stream;
  const int nk = g.nk;
  const size_t hpl = (size_t)g.nih * g.njh, upl = (size_t)(g.nih + 1) * g.njh, vpl = (size_t)g.nih * (g.njh + 1);
  const size_t fpl = upl > vpl ? upl : vpl;
  NDArgs A = {};
  A.E = EosDev{eos->form, eos->Rho_T0_S0, eos->dRho_dT, eos->dRho_dS};
  A.ref_pres = nd->ref_pres; A.gH = g.g_Earth * nd->H_to_RZ; A.pa_to_H = 1. / (nd->H_to_RZ * g.g_Earth);
  A.h_neglect = g.H_subroundoff; A.p_surf = c.p_surf; A.interior = nd->interior_only != 0; A.ebt = c.ebt_struct;
  const int coef = (taper ? ND_COEF_TAPER : 0) | (ebt ? ND_COEF_EBT : 0);
  const int ni = g.iec - g.isc + 1, nj = g.jec - g.jsc + 1;
  const int nbc = (ni + 2 + 63) / 64, nbu = (ni + 1 + 63) / 64, nbv = (ni + 63) / 64;      // blocks along i: columns with the halo, u faces, v faces
  const dim3 gc(nbc * (nj + 2)), gu(nbu * nj), gv(nbv * (nj + 1)), b64(64);
  NDBranch b;
  b.ns = 2 * nk + 2; b.flux_has_coef = ebt;
  b.bad = {{1, "ppm_ave: dx<0 or dx>1 should not happened! (a neutral layer spans more than one cell)"},
           {2, "neutral_diffusion: a neutral surface lies above the one before it in a column"}};
  b.scratch = [&](const double *hbl) -> int {
    A.hbl = hbl;
    A.irec = (double *)c.st.scratch(sizeof(double) * hpl * (nk + 1) * IREC);
    A.trec = (double *)c.st.scratch(sizeof(double) * hpl * ((size_t)nk + 1) * TREC);
    if (A.interior) { A.zbot = (double *)c.st.scratch(sizeof(double) * hpl); A.kbot = (int *)c.st.scratch(sizeof(int) * hpl); }
    if (ebt) A.coef_h = (double *)c.st.scratch(sizeof(double) * hpl * ((size_t)nk + 1));
    if (taper) { A.kt[0] = (ko_t *)c.st.scratch(sizeof(ko_t) * fpl * 8); A.kt[1] = A.kt[0] + fpl * 4; }
    M6_REQUIRE(!c.st.failed() && A.irec && A.trec && (!A.interior || (A.zbot && A.kbot)) && (!ebt || A.coef_h) && (!taper || A.kt[0]),
               "neutral_diffusion: out of device memory");
    return 0;
  };
  b.surfaces = [&]() -> int {
    A.T = c.d_tr[c.idx_T]; A.S = c.d_tr[c.idx_S];
    hipLaunchKernelGGL(nd_column_kernel, gc, b64, 0, s, A, nbc);
    hipLaunchKernelGGL(nd_surfaces_kernel<0>, gu, b64, 0, s, A, nbu);
    hipLaunchKernelGGL(nd_surfaces_kernel<1>, gv, b64, 0, s, A, nbv);
    if (taper) {      // the layer numbers of the taper depend on h and CS%hbl only: once where the surfaces are formed
      hipLaunchKernelGGL(nd_taper_kernel<0>, gu, b64, 0, s, A, nbu);
      hipLaunchKernelGGL(nd_taper_kernel<1>, gv, b64, 0, s, A, nbv);
    }
    return 0;
  };
  if (ebt) b.once = [&]() -> int {      // Coef_h :670-684 depends on khdt, I_numitts and ebt_struct only: once a call, not once an iteration
    M6_HIP(hipMemsetAsync(A.coef_h, 0, sizeof(double) * hpl * ((size_t)nk + 1), s));
    hipLaunchKernelGGL(nd_coef_h_kernel, dim3((ni + 63) / 64, nj), b64, 0, s, A);
    double *f1[1] = {A.coef_h}; int32_t p1[1] = {MOM6HIP_POS_H}, n1[1] = {nk + 1};
    return m6::group_pass(c.ctx, f1, p1, n1, 1);      // pass_var(CS%Coef_h, G%Domain)
  };
  b.tracer_cols = [&]() { hipLaunchKernelGGL(nd_tracer_cols_kernel, gc, b64, 0, s, A, nbc); };
  // the two flux kernels of a batch in the coefficient mode of the call
  // (tx, ty: the form that also leaves dfx_2d / dfy_2d, in the symmetric order only)
  auto launch_flux = [&](auto sym, auto mode, const NDTransOut *tx, const NDTransOut *ty) {
    constexpr bool SYM = decltype(sym)::value;
    constexpr int MODE = decltype(mode)::value;
    if constexpr (SYM) {
      if (tx) hipLaunchKernelGGL((nd_flux_kernel<0, true, MODE, NDTransOut>), gu, b64, 0, s, A, nbu, *tx);
      else hipLaunchKernelGGL((nd_flux_kernel<0, true, MODE>), gu, b64, 0, s, A, nbu);
      if (ty) hipLaunchKernelGGL((nd_flux_kernel<1, true, MODE, NDTransOut>), gv, b64, 0, s, A, nbv, *ty);
      else hipLaunchKernelGGL((nd_flux_kernel<1, true, MODE>), gv, b64, 0, s, A, nbv);
    } else {
      hipLaunchKernelGGL((nd_flux_kernel<0, false, MODE>), gu, b64, 0, s, A, nbu);
      hipLaunchKernelGGL((nd_flux_kernel<1, false, MODE>), gv, b64, 0, s, A, nbv);
    }
  };
  auto launch_fluxes = [&](auto sym, const NDTransOut *tx, const NDTransOut *ty) {
    if (coef == ND_COEF_NONE) launch_flux(sym, std::integral_constant<int, ND_COEF_NONE>(), tx, ty);
    else if (coef == ND_COEF_TAPER) launch_flux(sym, std::integral_constant<int, ND_COEF_TAPER>(), tx, ty);
    else if (coef == ND_COEF_EBT) launch_flux(sym, std::integral_constant<int, ND_COEF_EBT>(), tx, ty);
    else launch_flux(sym, std::integral_constant<int, ND_COEF_BOTH>(), tx, ty);
  };
  b.fluxes = [&](bool symmetric, const NDTransOut *tx, const NDTransOut *ty) {
    if (symmetric) launch_fluxes(std::true_type(), tx, ty); else launch_fluxes(std::false_type(), tx, ty);
  };
  return neutral_drive(c, nd, A, b);
}
}  // namespace m6
