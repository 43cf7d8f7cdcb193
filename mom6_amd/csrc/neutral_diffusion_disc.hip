// neutral_diffusion_disc.hip -- the discontinuous-reconstruction branch (NDIFF_CONTINUOUS = False) of MOM_neutral_diffusion
// (src/tracer/MOM_neutral_diffusion.F90) as gfx950 kernels, called from neutral_branch (neutral_diffusion.hip) when
// nd->unsupported[0] is set and the parameters of the branch (mom6hip_ndiff_discontinuous_cs_t) came with the call.  The branch supplies
// its kernels to neutral_drive (neutral_common.hpp), the host driver it shares with the continuous reconstruction.
//
//   ndd_column_kernel      neutral_diffusion_calc_coeffs :394-508 for one h column (halo 1): P_i(k,1:2) as :436-451 sums them,
//                          build_reconstructions_1d of T and S (remap_column.hpp), the edge values re-evaluated from the polynomial at 0
//                          and 1 (:467-472), mark_unstable_cells (:1841) and, with NDIFF_INTERIOR_ONLY, stable_cell(1:k_bot) = false
//                          (:500-506) -> thirteen planes [field][layer][h points].  dRdT_i / dRdS_i (:484-493) are never read: not formed
//   ndd_surfaces_kernel    find_neutral_surface_positions_discontinuous (:1604) for one face: the walk down the 4 nk surfaces with
//                          search_other_column (:1860), interpolate_for_nondim_position, find_neutral_pos_linear (:1964),
//                          find_neutral_pos_full (:2084) and calc_delta_rho_and_derivs (:2177); PoL, PoR, KoL, KoR, hEff (already in H
//                          units) as [surface][face] planes.  The call in calc_coeffs passes no k_bot / zeta_bot: the walk starts at the top
//   ndd_tracer_cols_kernel build_reconstructions_1d of the batch's tracers (neutral_surface_flux :2400-2403): the coefficients and the edge
//                          values Tid(k,1:2) as planes [tracer][field][layer][h points]
//   ndd_flux_kernel        neutral_surface_flux :2442-2471 for one face and the batch, with neutral_surface_T_eval (:2478) and khtr_ave = 1:
//                          the tendencies of the two cells of the face (the symmetric order) or the fluxes, laid out as nd_flux_kernel
//                          leaves them, so that the update kernels of neutral_diffusion.hip finish the step with nsurf = 4 nk.
// kl_left and kl_right only increase, the reset of HARD_FAIL_HEFF = False copies the layer number above, and the last surface is in
// layer nk: KoL and KoR never decrease, so a layer's sum is a run of consecutive surfaces here too (the `bad & 2` guard stays).
// Every plane covers the whole domain: 71-86 GB at 1440 x 1080 x 75 with 4 tracers, which runs on the card's 288 GB (158-242 ms a call,
// profiles/ndiff_discontinuous.txt); the branch is not tiled.
// A lane owns a column or a face.  The walk is serial and differs from lane to lane; the layer a side stands in is kept in registers
// and loaded again only when the walk enters another layer.
#include <cfloat>
#include <cmath>

#include "neutral_common.hpp"
#include "eos.hpp"
#define REMAP_PIECES_SELECT 1
#include "remap_pieces.hpp"
#include "remap_column.hpp"

namespace {

using namespace m6;
using namespace m6::eos;

constexpr int CREC = 13;      // a layer of a column: P_i(k,1:2), the coefficients of T and of S (three each), T_i(k,1:2), S_i(k,1:2), stable_cell
constexpr int QREC = 5;       // a layer of a column for one tracer: its coefficients (three) and Tid(k,1:2)

struct NDDArgs : NDFaces {
  EosDev E;
  double ref_pres, gH, h_neglect, drho_tol, x_tol;
  int scheme, nterm, method, imethod, form, max_iter, hard_fail, interior;      // method: NEUTRAL_POS_METHOD; imethod: the integration method
  const double *T, *S, *p_surf, *hbl;
  double *crec, *qrec;
};

__device__ __forceinline__ long crec_at(int q, int k, long c, long hpl, int nk) { return ((long)q * nk + k) * hpl + c; }
__device__ __forceinline__ long qrec_at(int z, int q, int k, long c, long hpl, int nk) { return (((long)z * QREC + q) * nk + k) * hpl + c; }

// evaluation_polynomial (src/ALE/polynomial_functions.F90:19) of two or three coefficients: x**0 is 1 for every x
__device__ __forceinline__ double eval_poly(const double c[3], int nterm, double x) {
  double f = 0.0;
  f = f + c[0] * 1.0;
  f = f + c[1] * x;
  if (nterm > 2) f = f + c[2] * (x * x);
  return f;
}
// first_derivative_polynomial :46
__device__ __forceinline__ double deriv_poly(const double c[3], int nterm, double x) {
  double f = 0.0;
  f = f + 1.0 * c[1] * 1.0;
  if (nterm > 2) f = f + 2.0 * c[2] * x;
  return f;
}

// build_reconstructions_1d (MOM_remapping.F90:257) without boundary extrapolation for PLM, PPM_H4 and PPM_IH4: EL, ER the edge values,
// C1 ppoly_coefs(:,2); ppoly_coefs(:,1) is EL and (:,3) is coef3() for a parabola and 0 otherwise.  Returns the integration method
template <int NKM>
__device__ int build_column(int scheme, int n, const double *h, const double *u, double *EL, double *ER, double *C1, double *w,
                            double h_neglect) {
  const int local = remap_local_scheme(scheme, n);
  if (local == MOM6HIP_REMAP_PCM) {
    for (int k = 0; k < n; k++) { EL[k] = u[k]; ER[k] = u[k]; C1[k] = 0.; }
    return INT_PCM;
  }
  if (local == MOM6HIP_REMAP_PLM) {
    plm_reconstruction(n, h, u, EL, ER, C1, h_neglect, w, w + n);
    return INT_PLM;
  }
  if (local == MOM6HIP_REMAP_PPM_H4) edge_values_explicit_h4(n, h, u, EL, ER, h_neglect);
  else edge_values_implicit_h4(n, h, u, EL, ER, h_neglect, w);
  ppm_reconstruction(n, h, u, EL, ER, C1);
  return INT_PPM;
}
// ppoly_coefs(k,3) of PPM_reconstruction (PPM_functions.F90:66)
__device__ __forceinline__ double coef3(int method, double u, double el, double er) {
  return method == INT_PPM ? 3.0 * ((er - u) + (el - u)) : 0.0;
}

// calc_delta_rho_and_derivs :2177 (the derivatives of point 1 and point 2 where the form has them)
__device__ __forceinline__ double calc_delta_rho(const NDDArgs &A, double T1, double S1, double p1_in, double T2, double S2, double p2_in,
                                                 double &drdt1, double &drds1, double &drdt2, double &drds2) {
  double p1, p2;
  if (A.ref_pres > 0.) { p1 = A.ref_pres; p2 = A.ref_pres; }
  else { p1 = p1_in; p2 = p2_in; }
  if (A.form == MOM6HIP_DELTA_RHO_FULL) {
    const double pmid = 0.5 * (p1 + p2);
    const double rho1 = eos_density(A.E, T1, S1, pmid);
    const double rho2 = eos_density(A.E, T2, S2, pmid);
    return rho1 - rho2;
  }
  if (A.form == MOM6HIP_DELTA_RHO_MID_PRESSURE) {
    double pmid = 0.5 * (p1 + p2);
    if (A.ref_pres >= 0) pmid = A.ref_pres;
    eos_density_derivs(A.E, T1, S1, pmid, drdt1, drds1);
    eos_density_derivs(A.E, T2, S2, pmid, drdt2, drds2);
  } else {
    eos_density_derivs(A.E, T1, S1, p1, drdt1, drds1);
    eos_density_derivs(A.E, T2, S2, p2, drdt2, drds2);
  }
  return 0.5 * ((drdt1 + drdt2) * (T1 - T2) + (drds1 + drds2) * (S1 - S2));      // delta_rho_from_derivs :2238
}
__device__ __forceinline__ double calc_delta_rho(const NDDArgs &A, double T1, double S1, double p1, double T2, double S2, double p2) {
  double a = 0., b = 0., c = 0., d = 0.;
  return calc_delta_rho(A, T1, S1, p1, T2, S2, p2, a, b, c, d);
}

// interpolate_for_nondim_position :1563
__device__ __forceinline__ double interp_nondim(double dRhoNeg, double Pneg, double dRhoPos, double Ppos) {
  if (Ppos <= Pneg) return 0.5;
  if (dRhoPos - dRhoNeg > 0.) return m6::min2(1., m6::max2(0., -dRhoNeg / (dRhoPos - dRhoNeg)));
  if (dRhoPos - dRhoNeg == 0) {
    if (dRhoNeg > 0.) return 0.;
    if (dRhoNeg < 0.) return 1.;
    return 0.5;
  }
  return 0.5;
}

// find_neutral_pos_linear :1964
__device__ double find_neutral_pos_linear(const NDDArgs &A, double z0, double T_ref, double S_ref, double dRdT_ref, double dRdS_ref,
                                          double dRdT_top, double dRdS_top, double dRdT_bot, double dRdS_bot, const double pT[3],
                                          const double pS[3], int &bad) {
  const int nterm = A.nterm;
  const double dRdT_diff = dRdT_bot - dRdT_top;
  const double dRdS_diff = dRdS_bot - dRdS_top;
  double zmin = z0, zmax = 1.;
  double a1 = 1. - zmin, a2 = zmin;
  double T_z = eval_poly(pT, nterm, zmin);
  double S_z = eval_poly(pS, nterm, zmin);
  double dRdT_z = a1 * dRdT_top + a2 * dRdT_bot;
  double dRdS_z = a1 * dRdS_top + a2 * dRdS_bot;
  double drho_min = 0.5 * ((dRdT_z + dRdT_ref) * (T_z - T_ref) + (dRdS_z + dRdS_ref) * (S_z - S_ref));
  T_z = eval_poly(pT, nterm, 1.);
  S_z = eval_poly(pS, nterm, 1.);
  double drho_max = 0.5 * ((dRdT_bot + dRdT_ref) * (T_z - T_ref) + (dRdS_bot + dRdS_ref) * (S_z - S_ref));
  if (drho_min >= 0.) return z0;
  else if (drho_max == 0.) return 1.;
  if (copysign(1., drho_min) == copysign(1., drho_max)) { bad |= 8; return z0; }
  double z = z0, ztest = z0;
  for (int iter = 1; iter <= A.max_iter; iter++) {
    a1 = 1. - z; a2 = z;
    dRdT_z = a1 * dRdT_top + a2 * dRdT_bot;
    dRdS_z = a1 * dRdS_top + a2 * dRdS_bot;
    T_z = eval_poly(pT, nterm, z);
    S_z = eval_poly(pS, nterm, z);
    const double drho = 0.5 * ((dRdT_z + dRdT_ref) * (T_z - T_ref) + (dRdS_z + dRdS_ref) * (S_z - S_ref));
    if (fabs(drho) <= A.drho_tol) break;
    if (drho < 0. && drho > drho_min) { drho_min = drho; zmin = z; }
    else if (drho > 0. && drho < drho_max) { drho_max = drho; zmax = z; }
    const double dT_dz = deriv_poly(pT, nterm, z);
    const double dS_dz = deriv_poly(pS, nterm, z);
    const double drho_dz = 0.5 * ((dRdT_diff * (T_z - T_ref) + (dRdT_ref + dRdT_z) * dT_dz) + (dRdS_diff * (S_z - S_ref) + (dRdS_ref + dRdS_z) * dS_dz));
    ztest = z - drho / drho_dz;
    if (ztest < zmin || ztest > zmax) {
      if (drho < 0.) ztest = 0.5 * (z + zmax);
      else ztest = 0.5 * (zmin + z);
    }
    if (fabs(z - ztest) <= A.x_tol) break;
    z = ztest;
  }
  return z;
}

// find_neutral_pos_full :2084
__device__ double find_neutral_pos_full(const NDDArgs &A, double z0, double T_ref, double S_ref, double P_ref, double P_top, double P_bot,
                                        const double pT[3], const double pS[3]) {
  const int nterm = A.nterm;
  int side = 0;
  double b = z0, c = 1.;
  const double Tb = eval_poly(pT, nterm, b);
  const double Sb = eval_poly(pS, nterm, b);
  const double Pb = P_top * (1. - b) + P_bot * b;
  double drho_b = calc_delta_rho(A, Tb, Sb, Pb, T_ref, S_ref, P_ref);
  const double Tc = eval_poly(pT, nterm, 1.);
  const double Sc = eval_poly(pS, nterm, 1.);
  const double Pc = P_bot;
  double drho_c = calc_delta_rho(A, Tc, Sc, Pc, T_ref, S_ref, P_ref);
  if (drho_b >= 0.) return z0;
  else if (drho_c == 0.) return 1.;
  if (copysign(1., drho_b) == copysign(1., drho_c)) return z0;
  double a = z0;
  for (int iter = 1; iter <= A.max_iter; iter++) {
    a = (drho_b * c - drho_c * b) / (drho_b - drho_c);
    const double Ta = eval_poly(pT, nterm, a);
    const double Sa = eval_poly(pS, nterm, a);
    const double Pa = P_top * (1. - a) + P_bot * a;
    const double drho_a = calc_delta_rho(A, Ta, Sa, Pa, T_ref, S_ref, P_ref);
    if (fabs(drho_a) < A.drho_tol) return a;
    if (drho_a * drho_c > 0.) {
      if (fabs(a - c) < A.x_tol) return a;
      c = a; drho_c = drho_a;
      if (side == -1) drho_b = 0.5 * drho_b;
      side = -1;
    } else if (drho_b * drho_a > 0) {
      if (fabs(a - b) < A.x_tol) return a;
      b = a; drho_b = drho_a;
      if (side == 1) drho_c = 0.5 * drho_c;
      side = 1;
    } else {
      return a;
    }
  }
  return a;
}

// the layer a side of the walk stands in
struct Lay { double P1, P2, T1, T2, S1, S2, cT[3], cS[3], h; bool stable; };

// search_other_column :1860 (ksurf 1-based): the position in the layer L of the interface (T_from, S_from, P_from)
__device__ double search_other_column(const NDDArgs &A, int ksurf, double pos_last, double T_from, double S_from, double P_from, const Lay &L,
                                      int &bad) {
  double dRdT_top = 0., dRdS_top = 0., dRdT_bot = 0., dRdS_bot = 0., dRdT_from = 0., dRdS_from = 0.;
  const double dRhoTop = calc_delta_rho(A, L.T1, L.S1, L.P1, T_from, S_from, P_from, dRdT_top, dRdS_top, dRdT_from, dRdS_from);
  const double dRhoBot = calc_delta_rho(A, L.T2, L.S2, L.P2, T_from, S_from, P_from, dRdT_bot, dRdS_bot, dRdT_from, dRdS_from);
  if (dRhoTop > 0. || ksurf == 1) return pos_last;
  else if (dRhoTop > dRhoBot) return 1.;
  else if (dRhoTop < 0. && dRhoBot < 0.) return 1.;
  else if (dRhoTop == 0. && dRhoBot == 0.) return 1.;
  else if (dRhoBot == 0.) return 1.;
  else if (dRhoTop == 0.) return pos_last;
  if (A.method == 1) return interp_nondim(dRhoTop, L.P1, dRhoBot, L.P2);
  if (A.method == 2)
    return find_neutral_pos_linear(A, pos_last, T_from, S_from, dRdT_from, dRdS_from, dRdT_top, dRdS_top, dRdT_bot, dRdS_bot, L.cT, L.cS, bad);
  return find_neutral_pos_full(A, pos_last, T_from, S_from, P_from, L.P1, L.P2, L.cT, L.cS);
}

template <int NKM>
__global__ __launch_bounds__(64) void ndd_column_kernel(NDDArgs A, int nbx) {
  const m6::GridDev &g = A.g;
  const NDCol C = nd_column(g, nbx);
  if (!C.has) return;
  const long n2 = C.n2, hpl = C.hpl;
  const int nk = g.nk;
  double h[NKM], u[NKM], EL[NKM], ER[NKM], C1[NKM], w[5 * (NKM + 1)];
  double *__restrict__ r = A.crec;
  for (int k = 0; k < nk; k++) h[k] = A.h[n2 + hpl * k];
  // P_i :436-451: the running sum starts again from P_i(k-1,2)
  double P2 = 0.;
  for (int k = 0; k < nk; k++) {
    double P1;
    if (k == 0) {
      if (A.p_surf) { P1 = A.p_surf[n2]; P2 = A.p_surf[n2] + h[0] * A.gH; }
      else { P1 = 0.; P2 = h[0] * A.gH; }
    } else { P1 = P2; P2 = P2 + h[k] * A.gH; }
    r[crec_at(0, k, n2, hpl, nk)] = P1; r[crec_at(1, k, n2, hpl, nk)] = P2;
  }
  for (int f = 0; f < 2; f++) {      // T, then S
    const double *__restrict__ src = f ? A.S : A.T;
    for (int k = 0; k < nk; k++) u[k] = src[n2 + hpl * k];
    const int method = build_column<NKM>(A.scheme, nk, h, u, EL, ER, C1, w, A.h_neglect);
    for (int k = 0; k < nk; k++) {
      const double c[3] = {EL[k], C1[k], coef3(method, u[k], EL[k], ER[k])};
      for (int q = 0; q < 3; q++) r[crec_at(2 + 3 * f + q, k, n2, hpl, nk)] = c[q];
      r[crec_at(8 + 2 * f, k, n2, hpl, nk)] = eval_poly(c, A.nterm, 0.);      // :467-472
      r[crec_at(9 + 2 * f, k, n2, hpl, nk)] = eval_poly(c, A.nterm, 1.);
    }
  }
  int k_bot = 0;
  if (A.interior) {      // :383-388, :500-506
    double zeta_bot;
    k_bot = 1;
    if (g.mask2dT[n2] > 0.0) boundary_k_range_surface(h, 1, nk, A.hbl[n2], k_bot, zeta_bot);
  }
  for (int k = 0; k < nk; k++) {      // mark_unstable_cells :1841
    const double P1 = r[crec_at(0, k, n2, hpl, nk)], Pb = r[crec_at(1, k, n2, hpl, nk)];
    const double d = calc_delta_rho(A, r[crec_at(9, k, n2, hpl, nk)], r[crec_at(11, k, n2, hpl, nk)], m6::max2(Pb, A.ref_pres),
                                    r[crec_at(8, k, n2, hpl, nk)], r[crec_at(10, k, n2, hpl, nk)], m6::max2(P1, A.ref_pres));
    r[crec_at(12, k, n2, hpl, nk)] = (d > 0. && k >= k_bot) ? 1.0 : 0.0;
  }
}

template <int DIR>
__global__ __launch_bounds__(64) void ndd_surfaces_kernel(NDDArgs A, int nbx) {
  const m6::GridDev &g = A.g;
  const NDFace F = nd_face<DIR>(g, nbx);
  if (!F.has) return;
  const long f = F.f, pl = F.pl, hpl = F.hpl, cl = F.cl, cr = F.cr;
  if (!F.wet) { nd_dry_surfaces<DIR>(A, f, pl); return; }
  double *__restrict__ PoL = A.PoL[DIR], *__restrict__ PoR = A.PoR[DIR], *__restrict__ hEff = A.hEff[DIR];
  ko_t *__restrict__ KoL = A.KoL[DIR], *__restrict__ KoR = A.KoR[DIR];
  const int ns = A.ns, nk = g.nk;
  const double *__restrict__ r = A.crec;
  auto load = [&](long c, int kl) {      // the layer kl (1-based) of the column c
    const int k = kl - 1;
    Lay L;
    L.P1 = r[crec_at(0, k, c, hpl, nk)]; L.P2 = r[crec_at(1, k, c, hpl, nk)];
    for (int q = 0; q < 3; q++) { L.cT[q] = r[crec_at(2 + q, k, c, hpl, nk)]; L.cS[q] = r[crec_at(5 + q, k, c, hpl, nk)]; }
    L.T1 = r[crec_at(8, k, c, hpl, nk)]; L.T2 = r[crec_at(9, k, c, hpl, nk)];
    L.S1 = r[crec_at(10, k, c, hpl, nk)]; L.S2 = r[crec_at(11, k, c, hpl, nk)];
    L.stable = r[crec_at(12, k, c, hpl, nk)] != 0.;
    L.h = A.h[c + hpl * k];
    return L;
  };
  int ki_right = 1, ki_left = 1, kl_left = 1, kl_right = 1;
  double lastP_left = 0., lastP_right = 0.;
  bool reached_bottom = false, s_left = false, s_right = false;
  Lay LL = load(cl, 1), LR = load(cr, 1);
  int bad = 0;
  // increment_interface :1931
  auto increment = [&](int &kl, int &ki, bool &this_col, bool &other_col) {
    reached_bottom = false;
    if (ki == 2) {
      if (kl < nk) { kl = kl + 1; ki = 1; }
      else { reached_bottom = true; this_col = false; other_col = true; }
    } else ki = 2;
  };
  double pL_prev = 0., pR_prev = 0.;
  int kL_prev = 1, kR_prev = 1;
  for (int ks = 1; ks <= ns; ks++) {
    double pL, pR;
    int oKL, oKR;
    if (ks == ns) { pL = 1.; pR = 1.; oKL = nk; oKR = nk; }
    else if (!LL.stable) {
      if (ks > 1) { pL = (double)(ki_left - 1); oKL = kl_left; pR = pR_prev; oKR = kR_prev; }
      else { pR = 0.; oKR = 1; pL = 0.; oKL = 1; }
      const int k0 = kl_left;
      increment(kl_left, ki_left, s_left, s_right);
      if (kl_left != k0) LL = load(cl, kl_left);
      s_left = true; s_right = false;
    } else if (!LR.stable) {
      if (ks > 1) { pR = (double)(ki_right - 1); oKR = kl_right; pL = pL_prev; oKL = kL_prev; }
      else { pR = 0.; oKR = 1; pL = 0.; oKL = 1; }
      const int k0 = kl_right;
      increment(kl_right, ki_right, s_right, s_left);
      if (kl_right != k0) LR = load(cr, kl_right);
      s_left = false; s_right = true;
    } else {
      const double TRi = (ki_right == 1) ? LR.T1 : LR.T2, SRi = (ki_right == 1) ? LR.S1 : LR.S2, PRi = (ki_right == 1) ? LR.P1 : LR.P2;
      const double TLi = (ki_left == 1) ? LL.T1 : LL.T2, SLi = (ki_left == 1) ? LL.S1 : LL.S2, PLi = (ki_left == 1) ? LL.P1 : LL.P2;
      const double dRho = calc_delta_rho(A, TRi, SRi, PRi, TLi, SLi, PLi);
      if (!reached_bottom) {
        if (dRho < 0.) { s_left = true; s_right = false; }
        else if (dRho > 0.) { s_left = false; s_right = true; }
        else if ((kl_left + kl_right == 2) && (ki_left + ki_right == 2)) { s_left = true; s_right = false; }
        else { s_left = !s_left; s_right = !s_right; }
      }
      if (s_left) {
        pR = (double)ki_right - 1.; oKR = kl_right;
        pL = search_other_column(A, ks, lastP_left, TRi, SRi, PRi, LL, bad);
        oKL = kl_left;
        const int k0 = kl_right;
        increment(kl_right, ki_right, s_right, s_left);
        if (kl_right != k0) LR = load(cr, kl_right);
        lastP_left = pL;
        if (kl_right == oKR + 1) lastP_right = 0.;
      } else {      // (searching_right_column: one of the two holds from the first surface on)
        pL = (double)ki_left - 1.; oKL = kl_left;
        pR = search_other_column(A, ks, lastP_right, TLi, SLi, PLi, LR, bad);
        oKR = kl_right;
        const int k0 = kl_left;
        increment(kl_left, ki_left, s_left, s_right);
        if (kl_left != k0) LL = load(cl, kl_left);
        lastP_right = pR;
        if (kl_left == oKL + 1) lastP_left = 0.;
      }
    }
    if (ks > 1) {      // the effective thickness :1806-1836 (hEff starts from 0, :510)
      double he = 0.;
      if (oKL == kL_prev && oKR == kR_prev) {
        const double hL = (pL - pL_prev) * A.h[cl + hpl * (oKL - 1)];
        const double hR = (pR - pR_prev) * A.h[cr + hpl * (oKR - 1)];
        if (hL < 0. || hR < 0.) {
          if (A.hard_fail) bad |= 4;
          if (s_left) { pL = pL_prev; oKL = kL_prev; }
          else if (s_right) { pR = pR_prev; oKR = kR_prev; }
        } else if (hL + hR == 0.) he = 0.;
        else he = 2. * ((hL * hR) / (hL + hR));
      }
      hEff[f + pl * (ks - 2)] = he;
    }
    PoL[f + pl * (ks - 1)] = pL; PoR[f + pl * (ks - 1)] = pR; KoL[f + pl * (ks - 1)] = (ko_t)oKL; KoR[f + pl * (ks - 1)] = (ko_t)oKR;
    pL_prev = pL; pR_prev = pR; kL_prev = oKL; kR_prev = oKR;
  }
  if (bad) atomicOr(A.bad, bad);
}

template <int NKM>
__global__ __launch_bounds__(64) void ndd_tracer_cols_kernel(NDDArgs A, int nbx) {
  const m6::GridDev &g = A.g;
  const NDCol C = nd_column(g, nbx);
  if (!C.has) return;
  const long n2 = C.n2, hpl = C.hpl;
  const int nk = g.nk;
  double h[NKM], u[NKM], EL[NKM], ER[NKM], C1[NKM], w[5 * (NKM + 1)];
  for (int k = 0; k < nk; k++) h[k] = A.h[n2 + hpl * k];
  for (int z = 0; z < A.nb; z++) {
    const double *__restrict__ t = A.t[z];
    for (int k = 0; k < nk; k++) u[k] = t[n2 + hpl * k];
    const int method = build_column<NKM>(A.scheme, nk, h, u, EL, ER, C1, w, A.h_neglect);
    for (int k = 0; k < nk; k++) {
      A.qrec[qrec_at(z, 0, k, n2, hpl, nk)] = EL[k]; A.qrec[qrec_at(z, 1, k, n2, hpl, nk)] = C1[k];
      A.qrec[qrec_at(z, 2, k, n2, hpl, nk)] = coef3(method, u[k], EL[k], ER[k]);
      A.qrec[qrec_at(z, 3, k, n2, hpl, nk)] = EL[k]; A.qrec[qrec_at(z, 4, k, n2, hpl, nk)] = ER[k];
    }
  }
}

// neutral_surface_T_eval :2478 for the sublayer between the positions pt and pb of the layer k (0-based) of the column c
struct TEval { double top, bot, sub, top_int, bot_int; };
__device__ __forceinline__ TEval t_eval(const NDDArgs &A, int z, long c, int k, double pt, double pb, long hpl, int nk) {
  const double *__restrict__ q = A.qrec;
  const double co[3] = {q[qrec_at(z, 0, k, c, hpl, nk)], q[qrec_at(z, 1, k, c, hpl, nk)], q[qrec_at(z, 2, k, c, hpl, nk)]};
  const double e1 = q[qrec_at(z, 3, k, c, hpl, nk)], e2 = q[qrec_at(z, 4, k, c, hpl, nk)];
  TEval r;
  if (pt == 0. && pb == 1.) { r.top = e1; r.bot = e2; }
  else {
    if (k > 0 && pt == 0.) r.top = q[qrec_at(z, 4, k - 1, c, hpl, nk)];
    else r.top = eval_poly(co, A.nterm, pt);
    if (k < nk - 1 && pb == 1.) r.bot = q[qrec_at(z, 3, k + 1, c, hpl, nk)];
    else r.bot = eval_poly(co, A.nterm, pb);
  }
  r.sub = average_value_ppoly(A.imethod, A.t[z][c + hpl * k], e1, e2, co[1], pt, pb);
  r.top_int = eval_poly(co, A.nterm, pt);
  r.bot_int = eval_poly(co, A.nterm, pb);
  return r;
}

// D: nothing, or (the symmetric order) one NDTransOut -- the form that also leaves trans_x_2d / trans_y_2d (:935-989).  The tracers of the
// batch are walked one after the other, each down the 4 nk surfaces, so the sum is one register
template <int DIR, bool SYM, typename... D>
__global__ __launch_bounds__(64) void ndd_flux_kernel(NDDArgs A, int nbx, D... d) {
  constexpr bool DIAG = sizeof...(D) > 0;
  static_assert(!DIAG || SYM, "the order of 2024 and before keeps the fluxes: nd_trans_march_kernel sums them");
  const m6::GridDev &g = A.g;
  const NDFace F = nd_face<DIR>(g, nbx);
  if (!F.has) return;
  const long f = F.f, pl = F.pl, hpl = F.hpl, cl = F.cl, cr = F.cr;
  const int ns = A.ns, nb = A.nb, nk = g.nk;
  if (!F.wet) {
    for (int z = 0; z < nb; z++)
      nd_dry_fluxes<SYM>(ns, nk, A.Flx[DIR] + A.flx_stride * z, A.tend[DIR][0] + A.flx_stride * z, A.tend[DIR][1] + A.flx_stride * z, f, pl);
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
  for (int z = 0; z < nb; z++) {
    double *__restrict__ Flx = SYM ? nullptr : A.Flx[DIR] + A.flx_stride * z;
    double *__restrict__ tdL = SYM ? A.tend[DIR][0] + A.flx_stride * z : nullptr, *__restrict__ tdR = SYM ? A.tend[DIR][1] + A.flx_stride * z : nullptr;
    double pLt = PiL[f], pRt = PiR[f];
    int klt = KoL[f] - 1, krt = KoR[f] - 1;
    double accL = 0., accR = 0.;
    [[maybe_unused]] double trans = 0.;
    if (SYM) { nd_tend_store(tdL, f, pl, -1, klt, 0.); nd_tend_store(tdR, f, pl, -1, krt, 0.); }
    for (int ks = 0; ks < ns - 1; ks++) {
      const double pLb = PiL[f + pl * (ks + 1)], pRb = PiR[f + pl * (ks + 1)];
      const int klb = KoL[f + pl * (ks + 1)] - 1, krb = KoR[f + pl * (ks + 1)] - 1;
      const double he = hEff[f + pl * ks];
      if (klb < klt || krb < krt) bad |= 2;      // (the positions of the surfaces never move up a column)
      double flx = 0.;
      if (he != 0.) {      // (then klb == klt and krb == krt: :1807)
        const TEval L = t_eval(A, z, cl, klt, pLt, pLb, hpl, nk), R = t_eval(A, z, cr, krt, pRt, pRb, hpl, nk);
        const double dT_top = R.top - L.top;
        const double dT_bottom = R.bot - L.bot;
        const double dT_sublayer = R.sub - L.sub;
        const double dT_top_int = R.top_int - L.top_int;
        const double dT_bot_int = R.bot_int - L.bot_int;
        bool down_flux = dT_top <= 0. && dT_bottom <= 0. && dT_sublayer <= 0. && dT_top_int <= 0. && dT_bot_int <= 0.;
        down_flux = down_flux || (dT_top >= 0. && dT_bottom >= 0. && dT_sublayer >= 0. && dT_top_int >= 0. && dT_bot_int >= 0.);
        if (down_flux) flx = dT_sublayer * he * 1.0;
      }
      if (SYM) { accL = accL + cf * flx; accR = accR - cf * flx; }
      else Flx[f + pl * ks] = flx;
      if constexpr (DIAG) trans = trans - cf * flx;
      if (SYM && klb > klt) { nd_tend_store(tdL, f, pl, klt, klb, accL); accL = 0.; }
      if (SYM && krb > krt) { nd_tend_store(tdR, f, pl, krt, krb, accR); accR = 0.; }
      pLt = pLb; pRt = pRb;
      if (klb > klt) klt = klb;
      if (krb > krt) krt = krb;
    }
    if (SYM) { nd_tend_store(tdL, f, pl, klt, nk, accL); nd_tend_store(tdR, f, pl, krt, nk, accR); }
    if constexpr (DIAG) {
      const NDTransOut &T = nd_first(d...);
      if (T.trans[z]) T.trans[z][f] = trans * T.Idt;
    }
  }
  if (bad) atomicOr(A.bad, bad);
}

template <int NKM>
void launch_columns(const NDDArgs &A, int nbc, int rows, hipStream_t s, bool tracers) {
  if (tracers) hipLaunchKernelGGL(ndd_tracer_cols_kernel<NKM>, dim3(nbc * rows), dim3(64), 0, s, A, nbc);
  else hipLaunchKernelGGL(ndd_column_kernel<NKM>, dim3(nbc * rows), dim3(64), 0, s, A, nbc);
}

}  // namespace

namespace m6 {

// neutral_branch (neutral_diffusion.hip) with NDIFF_CONTINUOUS = False; ndd holds the parameters of the branch
int neutral_disc_branch(const HordiffCall &c, const mom6hip_neutral_diffusion_cs_t *nd, const mom6hip_ndiff_discontinuous_cs_t *ndd) {
  M6_REQUIRE(ndd->initialized, "neutral_diffusion: the control structure of NDIFF_CONTINUOUS = False is not initialised");
  M6_REQUIRE(ndd->remap_scheme == MOM6HIP_REMAP_PLM || ndd->remap_scheme == MOM6HIP_REMAP_PPM_H4 || ndd->remap_scheme == MOM6HIP_REMAP_PPM_IH4,
             "neutral_diffusion: NDIFF_REMAPPING_SCHEME other than PLM, PPM_H4 or PPM_IH4 is not provided by libmom6hip");
  M6_REQUIRE(!ndd->boundary_extrap, "neutral_diffusion: NDIFF_BOUNDARY_EXTRAP = True is not provided by libmom6hip");
  M6_REQUIRE(ndd->remap_answer_date >= 20190101, "neutral_diffusion: REMAPPING_ANSWER_DATE < 20190101 is not provided by libmom6hip");
  M6_REQUIRE(ndd->neutral_pos_method >= 0 && ndd->neutral_pos_method <= 4, "Invalid option for NEUTRAL_POS_METHOD");      // :246
  M6_REQUIRE(ndd->neutral_pos_method >= 1 && ndd->neutral_pos_method <= 3,
             "neutral_diffusion: NEUTRAL_POS_METHOD = %d is not provided by libmom6hip (1, 2 and 3 are; the reference's search finds no "
             "position with 0 or 4)", ndd->neutral_pos_method);
  M6_REQUIRE(ndd->delta_rho_form >= MOM6HIP_DELTA_RHO_FULL && ndd->delta_rho_form <= MOM6HIP_DELTA_RHO_LOCAL_PRESSURE, "delta_rho_form is not recognized");
  M6_REQUIRE(!(ndd->neutral_pos_method == 2 && ndd->delta_rho_form == MOM6HIP_DELTA_RHO_FULL),
             "neutral_diffusion: NEUTRAL_POS_METHOD = 2 with DELTA_RHO_FORM = full is not provided by libmom6hip (the reference reads density "
             "derivatives this form never sets)");
  M6_REQUIRE(!nd->unsupported[2], "neutral_diffusion: NDIFF_TAPERING with NDIFF_CONTINUOUS = False is not provided by libmom6hip");
  M6_REQUIRE(!nd->unsupported[3], "neutral_diffusion: KHTR_USE_EBT_STRUCT with NDIFF_CONTINUOUS = False is not provided by libmom6hip");
  M6_REQUIRE(ndd->neutral_pos_method == 1 || ndd->max_iter >= 0, "neutral_diffusion: NDIFF_MAX_ITER must not be negative");
  const m6::GridDev g = c.ctx->g;
  hipStream_t s = c.ctx->stream;
  const int nk = g.nk, ntr = (int)c.d_tr.size();
  const size_t hpl = (size_t)g.nih * g.njh;
  NDDArgs A = {};
  A.E = EosDev{c.eos->form, c.eos->Rho_T0_S0, c.eos->dRho_dT, c.eos->dRho_dS};
  A.ref_pres = nd->ref_pres; A.gH = g.g_Earth * nd->H_to_RZ; A.h_neglect = g.H_subroundoff;
  A.drho_tol = ndd->drho_tol; A.x_tol = ndd->x_tol; A.scheme = ndd->remap_scheme;
  A.nterm = ndd->remap_scheme == MOM6HIP_REMAP_PLM ? 2 : 3;      // CS%deg + 1
  A.form = ndd->delta_rho_form; A.max_iter = ndd->max_iter; A.hard_fail = ndd->hard_fail_heff != 0;
  A.method = ndd->neutral_pos_method; A.interior = nd->interior_only != 0; A.p_surf = c.p_surf;
  const int ni = g.iec - g.isc + 1, nj = g.jec - g.jsc + 1;
  const int nbc = (ni + 2 + 63) / 64, nbu = (ni + 1 + 63) / 64, nbv = (ni + 63) / 64;
  const dim3 gu(nbu * nj), gv(nbv * (nj + 1)), b64(64);
  auto columns = [&](bool tracers) {
    if (nk <= 32) launch_columns<32>(A, nbc, nj + 2, s, tracers);
    else if (nk <= 80) launch_columns<80>(A, nbc, nj + 2, s, tracers);
    else launch_columns<128>(A, nbc, nj + 2, s, tracers);
  };
  NDBranch b;
  b.ns = 4 * nk; b.flux_has_coef = false;
  b.bad = {{4, "Negative thicknesses in neutral diffusion"},      // :1812 (HARD_FAIL_HEFF)
           {8, "drho_min is the same sign as dhro_max"},          // :2032
           {2, "neutral_diffusion: a neutral surface lies above the one before it in a column"}};
  b.scratch = [&](const double *hbl) -> int {      // (the driver has checked nk by now)
    A.hbl = hbl;
    const int local = remap_local_scheme(ndd->remap_scheme, nk);      // the integration method build_reconstructions_1d returns on nk cells
    A.imethod = local == MOM6HIP_REMAP_PCM ? INT_PCM : local == MOM6HIP_REMAP_PLM ? INT_PLM : INT_PPM;
    A.crec = (double *)c.st.scratch(sizeof(double) * hpl * nk * CREC);
    A.qrec = (double *)c.st.scratch(sizeof(double) * hpl * nk * QREC * (size_t)(ntr < ND_BATCH ? ntr : ND_BATCH));
    M6_REQUIRE(!c.st.failed() && A.crec && A.qrec, "neutral_diffusion: out of device memory");
    return 0;
  };
  b.surfaces = [&]() -> int {
    A.T = c.d_tr[c.idx_T]; A.S = c.d_tr[c.idx_S];
    columns(false);
    hipLaunchKernelGGL(ndd_surfaces_kernel<0>, gu, b64, 0, s, A, nbu);
    hipLaunchKernelGGL(ndd_surfaces_kernel<1>, gv, b64, 0, s, A, nbv);
    return 0;
  };
  b.tracer_cols = [&]() { columns(true); };
  b.fluxes = [&](bool symmetric, const NDTransOut *tx, const NDTransOut *ty) {
    if (symmetric) {
      if (tx) hipLaunchKernelGGL((ndd_flux_kernel<0, true, NDTransOut>), gu, b64, 0, s, A, nbu, *tx);
      else hipLaunchKernelGGL((ndd_flux_kernel<0, true>), gu, b64, 0, s, A, nbu);
      if (ty) hipLaunchKernelGGL((ndd_flux_kernel<1, true, NDTransOut>), gv, b64, 0, s, A, nbv, *ty);
      else hipLaunchKernelGGL((ndd_flux_kernel<1, true>), gv, b64, 0, s, A, nbv);
    } else {
      hipLaunchKernelGGL((ndd_flux_kernel<0, false>), gu, b64, 0, s, A, nbu);
      hipLaunchKernelGGL((ndd_flux_kernel<1, false>), gv, b64, 0, s, A, nbv);
    }
  };
  return neutral_drive(c, nd, A, b);
}

}  // namespace m6

extern "C" uint64_t mom6hip_abi_sizeof_ndiff_discontinuous_cs(void) { return sizeof(mom6hip_ndiff_discontinuous_cs_t); }
