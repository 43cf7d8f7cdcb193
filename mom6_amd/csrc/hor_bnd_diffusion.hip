// hor_bnd_diffusion.hip -- horizontal boundary diffusion of tracers, USE_HORIZONTAL_BOUNDARY_DIFFUSION
// (src/tracer/MOM_hor_bnd_diffusion.F90; called by tracer_hordiff, MOM_tracer_hor_diff.F90:408-472), as gfx950 kernels.
//
//   hbd_count_kernel   per wet face: the size of its HBD grid (merge_interfaces :517, hbd_grid :343) and the number of leading native
//                      layers whose centre lies above htot_max (the layers that can carry a flux, :815-821); the maxima of both over
//                      the tile size the scratch planes below
//   hbd_setup_kernel   per wet face: the HBD grid dz_top and the diffusivity remapped onto it (khtr_ul_z, :760-769) -- both depend on
//                      h and hbl only, so they are formed once per call
//   hbd_flux_kernel    per wet face and tracer: fluxes_layer_method (:677-828) -- the two columns remapped onto dz_top, the layer
//                      fluxes above k_bot_min (with HBD_LINEAR_TRANSITION and APPLY_LIMITER_REMAP), reintegrate_column back onto
//                      the harmonic-mean thicknesses, APPLY_LIMITER (flux_limiter :576) and the cut below htot_max
//   hbd_update_kernel  the update of every layer of every wet cell (:262-270) and the concentration underflow (:274-278); fluxes of
//                      layers at or below a face's last flux layer are zero, so a layer no face reaches still gets t + 0
//                      (which turns a -0.0 into +0.0 as the reference does)
//   hbd_face_diag_kernel, hbd_update_kernel<HBDMixOut>  the hbd_* diagnostics (:292-333) where mom6hip_tracer_hordiff_mix_diag asks for
//                      them: the fluxes times Idt with their sums over k in layer order, and the content / concentration tendencies
// One lane per face walks the serial depth loops of its column pair from private arrays (sized by the template's layer bound NKM).
// The vertical reconstructions are those of remapping_core_h (src/ALE/MOM_remapping.F90:160) for PCM, PLM, PPM_H4, PPM_IH4 and
// PPM_CW, with and without boundary extrapolation, force_bounds_in_subcell = .false.  Their per-cell arithmetic lives in
// remap_pieces.hpp, the text the ALE kernels (ale_remap.hip) use too, here with minima and maxima by compare-and-select; the column
// drivers below are the serial loops over those pieces, on ALE's column layout (the edge values EL, ER and the slope column C1).
// (Five pieces are called from here alone, and ale_remap.hip's wave path keeps the same arithmetic in place; the header names them.)
// Algorithmic traffic per tracer and iteration: the flux kernels read h and the tracer of both columns of every wet face down to the
// HBD grid's depth and write nflx_max planes of fluxes per direction; the update reads h and the fluxes and reads and writes every
// layer of the tracer (>= 24 B per cell).
#include <cfloat>
#include <cmath>

#include "flux_diag_march.hpp"
#include "neutral_common.hpp"      // boundary_k_range_surface, the layer search neutral diffusion's NDIFF_INTERIOR_ONLY shares
#define REMAP_PIECES_SELECT 1      // m6::min2 / max2, as the oracle (remap_pieces.hpp says why there are two flavours)
#include "remap_pieces.hpp"
#include "remap_column.hpp"

namespace {

using m6::max2;
using m6::min2;

// the private work space of one remapping_core_h of at most NKM source and 2 NKM + 2 target cells
template <int NKM>
struct RemapWork {
  static constexpr int N1M = 2 * NKM + 2, NS = NKM + N1M + 3;
  double EL[NKM], ER[NKM], C1[NKM], w[5 * (NKM + 1)];
  double h_sub[NS], uh_sub[NS], u_sub[NS], h0_eff[NKM + 2];
  int isub_src[NS], isrc_start[NKM + 2], isrc_end[NKM + 2], isrc_max[NKM + 2], itgt_start[N1M + 2], itgt_end[N1M + 2];
};

// build_reconstructions_1d (:257-386) for the schemes provided; returns the integration method
template <int NKM>
__device__ int build_reconstructions(RemapWork<NKM> &W, int scheme, bool extrap, int n, const double *h0, const double *u0,
                                     double h_neglect, double h_neglect_edge) {
  const int local = remap_local_scheme(scheme, n);
  if (local == MOM6HIP_REMAP_PCM) {
    for (int k = 0; k < n; k++) { W.EL[k] = u0[k]; W.ER[k] = u0[k]; W.C1[k] = 0.; }
    return INT_PCM;
  }
  if (local == MOM6HIP_REMAP_PLM) {
    plm_reconstruction(n, h0, u0, W.EL, W.ER, W.C1, h_neglect, W.w, W.w + n);
    if (extrap) plm_boundary_extrapolation(h0, u0, W.EL, W.ER, W.C1, n, h_neglect);
    return INT_PLM;
  }
  if (local == MOM6HIP_REMAP_PPM_H4) edge_values_explicit_h4(n, h0, u0, W.EL, W.ER, h_neglect_edge);
  else if (local == MOM6HIP_REMAP_PPM_IH4) edge_values_implicit_h4(n, h0, u0, W.EL, W.ER, h_neglect_edge, W.w);
  else { edge_values_explicit_h4cw(n, h0, u0, W.EL, W.ER, h_neglect_edge, W.w); ppm_monotonicity(n, u0, W.EL, W.ER); }
  ppm_reconstruction(n, h0, u0, W.EL, W.ER, W.C1);
  if (extrap) ppm_boundary_extrapolation(h0, u0, W.EL, W.ER, W.C1, n, h_neglect);
  return INT_PPM;
}

// remap_via_sub_cells (:463-852) with force_bounds_in_subcell = .false. (n1 >= 1)
template <int NKM>
__device__ void remap_via_sub_cells(RemapWork<NKM> &W, int n0, const double *h0, const double *u0, int n1, const double *h1, int method,
                                    double *u1) {
  const int ns = n0 + n1 + 1;
  double *h_sub = W.h_sub, *uh_sub = W.uh_sub, *u_sub = W.u_sub, *h0_eff = W.h0_eff;
  int *isub_src = W.isub_src, *isrc_start = W.isrc_start, *isrc_end = W.isrc_end, *isrc_max = W.isrc_max;
  int *itgt_start = W.itgt_start, *itgt_end = W.itgt_end;
#define H0(i) h0[(i) - 1]
#define H1(i) h1[(i) - 1]
#define U0(i) u0[(i) - 1]
  for (int i = 0; i <= ns + 1; i++) { h_sub[i] = 0.; uh_sub[i] = 0.; u_sub[i] = 0.; isub_src[i] = 0; }
  for (int i = 0; i <= n0 + 1; i++) { isrc_start[i] = 0; isrc_end[i] = 0; isrc_max[i] = 0; h0_eff[i] = 0.; }
  for (int i = 0; i <= n1 + 1; i++) { itgt_start[i] = 0; itgt_end[i] = 0; }
  int i0_last_thick_cell = 0;
  for (int i0 = 1; i0 <= n0; i0++)
    if (H0(i0) > 0.) i0_last_thick_cell = i0;
  double h0_supply = H0(1), h1_supply = H1(1);
  bool src_has_volume = true, tgt_has_volume = true;
  int i0 = 1, i1 = 1, i_start0 = 1, i_start1 = 1, i_max = 1;
  double dh_max = 0., dh0_eff = 0., dh;
  h_sub[1] = 0.;
  isrc_start[1] = 1; isrc_end[1] = 1; isrc_max[1] = 1; isub_src[1] = 1;
  for (int i_sub = 2; i_sub <= ns; i_sub++) {
    dh = min2(h0_supply, h1_supply);
    dh0_eff = dh0_eff + min2(dh, h0_supply);
    isub_src[i_sub] = i0;
    h_sub[i_sub] = dh;
    if (dh >= dh_max) { i_max = i_sub; dh_max = dh; }
    if (h0_supply <= h1_supply && src_has_volume) {
      h1_supply = h1_supply - dh;
      isrc_start[i0] = i_start0; isrc_end[i0] = i_sub; i_start0 = i_sub + 1;
      isrc_max[i0] = i_max; i_max = i_sub + 1; dh_max = 0.;
      h0_eff[i0] = dh0_eff;
      if (i0 < n0) { i0 = i0 + 1; h0_supply = H0(i0); dh0_eff = 0.; }
      else { h0_supply = 0.; src_has_volume = false; }
    } else if (h0_supply >= h1_supply && tgt_has_volume) {
      h0_supply = h0_supply - dh;
      itgt_start[i1] = i_start1; itgt_end[i1] = i_sub; i_start1 = i_sub + 1;
      if (i1 < n1) { i1 = i1 + 1; h1_supply = H1(i1); }
      else { h1_supply = 0.; tgt_has_volume = false; }
    } else if (src_has_volume) {
      h_sub[i_sub] = h0_supply;
      isrc_start[i0] = i_start0; isrc_end[i0] = i_sub; i_start0 = i_sub + 1;
      isrc_max[i0] = i_max; i_max = i_sub + 1; dh_max = 0.;
      h0_eff[i0] = dh0_eff;
      if (i0 < n0) { i0 = i0 + 1; h0_supply = H0(i0); dh0_eff = 0.; }
      else { h0_supply = 0.; src_has_volume = false; }
    } else if (tgt_has_volume) {
      h_sub[i_sub] = h1_supply;
      itgt_start[i1] = i_start1; itgt_end[i1] = i_sub; i_start1 = i_sub + 1;
      if (i1 < n1) { i1 = i1 + 1; h1_supply = H1(i1); }
      else { h1_supply = 0.; tgt_has_volume = false; }
    }
  }
  double xa = 0., xb;
  dh0_eff = 0.;
  uh_sub[1] = 0.;
  u_sub[1] = W.EL[0];
  for (int i_sub = 2; i_sub <= n0 + n1; i_sub++) {
    dh = h_sub[i_sub];
    i0 = isub_src[i_sub];
    dh0_eff = dh0_eff + dh;
    if (h0_eff[i0] > 0.) {
      xb = dh0_eff / h0_eff[i0];
      xb = min2(1., xb);
      u_sub[i_sub] = average_value_ppoly(method, U0(i0), W.EL[i0 - 1], W.ER[i0 - 1], W.C1[i0 - 1], xa, xb);
    } else {
      xb = 1.;
      u_sub[i_sub] = U0(i0);
    }
    uh_sub[i_sub] = dh * u_sub[i_sub];
    if (isub_src[i_sub + 1] != i0) { dh0_eff = 0.; xa = 0.; }
    else { xa = xb; }
  }
  u_sub[ns] = W.ER[n0 - 1];
  uh_sub[ns] = W.ER[n0 - 1] * h_sub[ns];
  for (i0 = 1; i0 <= i0_last_thick_cell; i0++) {      // adjust_thickest_subcell
    i_max = isrc_max[i0];
    dh_max = h_sub[i_max];
    if (dh_max > 0.) {
      double duh = 0.;
      for (int i_sub = isrc_start[i0]; i_sub <= isrc_end[i0]; i_sub++)
        if (i_sub != i_max) duh = duh + uh_sub[i_sub];
      uh_sub[i_max] = U0(i0) * H0(i0) - duh;
    }
  }
  for (i1 = 1; i1 <= n1; i1++) {
    if (H1(i1) > 0.) {
      double duh = 0.;
      dh = 0.;
      int i_sub = itgt_start[i1];
      double u1min = u_sub[i_sub], u1max = u_sub[i_sub];
      for (i_sub = itgt_start[i1]; i_sub <= itgt_end[i1]; i_sub++) {
        u1min = min2(u1min, u_sub[i_sub]);
        u1max = max2(u1max, u_sub[i_sub]);
        dh = dh + h_sub[i_sub];
        duh = duh + uh_sub[i_sub];
      }
      u1[i1 - 1] = duh / dh;
      u1[i1 - 1] = max2(u1min, min2(u1max, u1[i1 - 1]));
    } else {
      u1[i1 - 1] = u_sub[itgt_start[i1]];
    }
  }
#undef H0
#undef H1
#undef U0
}

template <int NKM>
__device__ void remapping_core_h(RemapWork<NKM> &W, int scheme, bool extrap, int n0, const double *h0, const double *u0, int n1,
                                 const double *h1, double *u1, double h_neglect) {
  const int method = build_reconstructions<NKM>(W, scheme, extrap, n0, h0, u0, h_neglect, h_neglect);
  remap_via_sub_cells<NKM>(W, n0, h0, u0, n1, h1, method, u1);
}

// reintegrate_column, src/ALE/MOM_remapping.F90:925-993
__device__ void reintegrate_column(int nsrc, const double *h_src, const double *uh_src, int ndest, const double *h_dest, double *uh_dest) {
  for (int k = 0; k < ndest; k++) uh_dest[k] = 0.0;
  int k_src = 0, k_dest = 0;
  double h_dest_rem = 0., h_src_rem = 0., uh_src_rem = 0., dh, duh;
  bool src_ran_out = false;
  while (true) {
    if (h_src_rem == 0. && k_src < nsrc) {
      k_src = k_src + 1;
      h_src_rem = h_src[k_src - 1];
      uh_src_rem = uh_src[k_src - 1];
      if (h_src_rem == 0.) continue;
    }
    if (h_dest_rem == 0. && k_dest < ndest) {
      k_dest = k_dest + 1;
      h_dest_rem = h_dest[k_dest - 1];
      uh_dest[k_dest - 1] = 0.;
      if (h_dest_rem == 0.) continue;
    }
    if (k_src == nsrc && h_src_rem == 0.) {
      if (src_ran_out) break;
      src_ran_out = true;
      continue;
    }
    duh = 0.;
    if (h_src_rem < h_dest_rem) {
      dh = h_src_rem;
      if (dh > 0.) duh = uh_src_rem;
      h_src_rem = 0.;
      uh_src_rem = 0.;
      h_dest_rem = max2(0., h_dest_rem - dh);
    } else if (h_src_rem > h_dest_rem) {
      dh = h_dest_rem;
      duh = (dh / h_src_rem) * uh_src_rem;
      h_src_rem = max2(0., h_src_rem - dh);
      uh_src_rem = uh_src_rem - duh;
      h_dest_rem = 0.;
    } else {
      duh = uh_src_rem;
      h_src_rem = 0.;
      uh_src_rem = 0.;
      h_dest_rem = 0.;
    }
    uh_dest[k_dest - 1] = uh_dest[k_dest - 1] + duh;
    if (k_dest == ndest && (k_src == nsrc || h_dest_rem == 0.)) break;
  }
}

// flux_limiter :576-605 (SIGN(1., x) as copysign: a -0.0 is negative)
__device__ __forceinline__ double flux_limiter(double F_layer, double area_L, double area_R, double phi_L, double phi_R, double h_L, double h_R) {
  const double F_max = -0.2 * ((area_R * (phi_R * h_R)) - (area_L * (phi_L * h_L)));
  if (copysign(1., F_layer) == copysign(1., F_max)) {
    if (F_max >= 0.) return min2(F_layer, F_max);
    return max2(F_layer, F_max);
  }
  return 0.0;
}

struct HBDArgs {
  m6::GridDev g;
  const double *h, *hbl, *khdt[2];
  const double *ebt;           // KHTR_USE_EBT_STRUCT: VarMix%ebt_struct [layer][h points] (null: off)
  double KhTr_min;             // KHTR_MIN, the floor of the interface coefficients below the first with FULL_DEPTH_KHTR_MIN
  int full_depth_khtr_min;
  double I_numitts, h_neglect;
  int linear, limiter, limiter_remap, extrap, scheme;
  int *kmax[2], *nflx[2];      // per face
  int *maxes;                  // [4]: kmax_max u, v; nflx_max u, v
  int nflx_max[2];
  double *dz[2], *khz[2];      // [kmax_max][faces]
  double *flx[2];              // [nflx_max][faces]
  double *t;                   // the tracer of the launch
  double cu;                   // its conc_underflow
};

// the faces of direction DIR: u faces (I, j), I = isc-1 .. iec, j = jsc .. jec; v faces (i, J), i = isc .. iec, J = jsc-1 .. jec.
// in_range: the thread has a face; the return value: the face is wet
template <int DIR>
__device__ __forceinline__ bool hbd_face(const m6::GridDev &g, bool &in_range, long &f, long &cL, long &cR) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (DIR == 0) {
    const int I = g.isc - 1 + x, j = g.jsc + y;
    in_range = I <= g.iec && j <= g.jec;
    if (!in_range) return false;
    f = g.u2(I, j); cL = g.h2(I, j); cR = g.h2(I + 1, j);
    return g.mask2dCu[f] > 0.;
  }
  const int i = g.isc + x, J = g.jsc - 1 + y;
  in_range = i <= g.iec && J <= g.jec;
  if (!in_range) return false;
  f = g.v2(i, J); cL = g.h2(i, J); cR = g.h2(i, J + 1);
  return g.mask2dCv[f] > 0.;
}

__device__ __forceinline__ long face_plane(const m6::GridDev &g, int dir) { return dir == 0 ? (long)(g.nih + 1) * g.njh : (long)g.nih * (g.njh + 1); }

// merge_interfaces :517-573: the distinct values of {0, eta_L(2:nk+1), eta_R(2:nk+1), hbl_L, hbl_R} in ascending order up to
// min(min(column depths), max(hbl_L, hbl_R)); the columns' interfaces are sorted already, so the sort is a merge of the three sorted
// lists (the same values, copied without arithmetic).  emit(k, dz) is called for every cell of the HBD grid; returns their number.
template <typename Emit>
__device__ int merge_interfaces(int nk, const double *h, long cL, long cR, long hpl, double hbl_L, double hbl_R, double Hs, Emit emit) {
  double eL = 0., eR = 0.;
  for (int k = 0; k < nk; k++) { eL = eL + h[cL + hpl * k]; eR = eR + h[cR + hpl * k]; }
  const double max_depth = min2(min2(eL, eR), max2(hbl_L, hbl_R));
  const double b[2] = {min2(hbl_L, hbl_R), max2(hbl_L, hbl_R)};
  int kL = 0, kR = 0, kb = 0, nout = 0;      // heads: eta_L(kL + 1), eta_R(kR + 1), b[kb]
  double vL = 0., vR = 0., last = 0.;
  bool first = true;
  while (true) {
    double v = INFINITY;
    int src = -1;
    if (kL <= nk && vL < v) { v = vL; src = 0; }
    if (kR <= nk && vR < v) { v = vR; src = 1; }
    if (kb < 2 && b[kb] < v) { v = b[kb]; src = 2; }
    if (src < 0 || !(v <= max_depth)) break;
    if (src == 0) { kL++; if (kL <= nk) vL = vL + h[cL + hpl * (kL - 1)]; }
    else if (src == 1) { kR++; if (kR <= nk) vR = vR + h[cR + hpl * (kR - 1)]; }
    else kb++;
    if (first) { first = false; last = v; continue; }
    if (v > last) { emit(nout, (v - last) + Hs); nout++; last = v; }
  }
  return nout;
}

// the number of leading layers whose centre lies at or above htot_max (:815-821); 0 if either boundary layer is empty
__device__ int flux_layers(int nk, const double *h, long cL, long cR, long hpl, double hbl_L, double hbl_R, bool linear) {
  if (hbl_L == 0. || hbl_R == 0.) return 0;
  const double htot_max = linear ? max2(hbl_L, hbl_R) : min2(hbl_L, hbl_R);
  double tmp1 = 0.0, tmp2 = 0.0;
  for (int k = 0; k < nk; k++) {
    const double hL = h[cL + hpl * k], hR = h[cR + hpl * k];
    if (max2(tmp1 + (hL * 0.5), tmp2 + (hR * 0.5)) > htot_max) return k;
    tmp1 = tmp1 + hL;
    tmp2 = tmp2 + hR;
  }
  return nk;
}

template <int DIR>
__global__ __launch_bounds__(64) void hbd_count_kernel(HBDArgs A) {
  const m6::GridDev &g = A.g;
  long f = 0, cL = 0, cR = 0;
  bool in_range;
  const bool wet = hbd_face<DIR>(g, in_range, f, cL, cR);
  if (!in_range) return;
  int km = 0, nf = 0;
  if (wet) {
    const long hpl = (long)g.nih * g.njh;
    km = merge_interfaces(g.nk, A.h, cL, cR, hpl, A.hbl[cL], A.hbl[cR], A.h_neglect, [](int, double) {});
    nf = km > 0 ? flux_layers(g.nk, A.h, cL, cR, hpl, A.hbl[cL], A.hbl[cR], A.linear != 0) : 0;
  }
  A.kmax[DIR][f] = km; A.nflx[DIR][f] = nf;
  if (km > 0) atomicMax(A.maxes + DIR, km);
  if (nf > 0) atomicMax(A.maxes + 2 + DIR, nf);
}

template <int NKM, int DIR>
__global__ __launch_bounds__(64) void hbd_setup_kernel(HBDArgs A) {
  const m6::GridDev &g = A.g;
  long f = 0, cL = 0, cR = 0;
  bool in_range;
  if (!hbd_face<DIR>(g, in_range, f, cL, cR)) return;
  const int km = A.kmax[DIR][f];
  if (km == 0) return;
  const long hpl = (long)g.nih * g.njh, fpl = face_plane(g, DIR);
  const int nk = g.nk;
  double *dz = A.dz[DIR];
  merge_interfaces(nk, A.h, cL, cR, hpl, A.hbl[cL], A.hbl[cR], A.h_neglect, [&](int k, double d) { dz[f + fpl * k] = d; });
  if (A.nflx[DIR][f] == 0) return;      // no fluxes through this face: khtr_ul_z is not read
  double h_vel[NKM], khtr_ul[NKM], dzl[2 * NKM + 2], khz[2 * NKM + 2];
  RemapWork<NKM> W;
  // Coef_x(I,j,K), MOM_tracer_hor_diff.F90:414-462: the same at every interface, or with KHTR_USE_EBT_STRUCT scaled below the first by
  // the mean of ebt_struct in the two columns and, with FULL_DEPTH_KHTR_MIN, floored by KHTR_MIN (compared as the reference writes it)
  const double c = A.I_numitts * A.khdt[DIR][f];
  double ku = c;      // khtr_u(k)
  for (int k = 0; k < nk; k++) {
    const double h1 = A.h[cL + hpl * k], h2 = A.h[cR + hpl * k];
    h_vel[k] = (h1 + h2 == 0.) ? 0. : 2. * (h1 * h2) / (h1 + h2);      // harmonic_mean :409
    double kn = c;      // khtr_u(k+1)
    if (A.ebt) {
      kn = c * 0.5 * (A.ebt[cL + hpl * k] + A.ebt[cR + hpl * k]);
      if (A.full_depth_khtr_min) kn = max2(kn, A.KhTr_min);
    }
    khtr_ul[k] = ku + 0.5 * (kn - ku);
    ku = kn;
  }
  for (int k = 0; k < km; k++) dzl[k] = dz[f + fpl * k];
  remapping_core_h<NKM>(W, A.scheme, A.extrap != 0, nk, h_vel, khtr_ul, km, dzl, khz, A.h_neglect);
  for (int k = 0; k < km; k++) A.khz[DIR][f + fpl * k] = khz[k];
}

template <int NKM, int DIR>
__global__ __launch_bounds__(64) void hbd_flux_kernel(HBDArgs A) {
  const m6::GridDev &g = A.g;
  long f = 0, cL = 0, cR = 0;
  bool in_range;
  const bool wet = hbd_face<DIR>(g, in_range, f, cL, cR);
  if (!in_range) return;
  const long hpl = (long)g.nih * g.njh, fpl = face_plane(g, DIR);
  const int nk = g.nk, nmax = A.nflx_max[DIR];
  double *flx = A.flx[DIR];
  const int nf = wet ? A.nflx[DIR][f] : 0;
  if (nf == 0) {
    for (int k = 0; k < nmax; k++) flx[f + fpl * k] = 0.0;
    return;
  }
  const int km = A.kmax[DIR][f];
  const double hbl_L = A.hbl[cL], hbl_R = A.hbl[cR];
  const double area_L = g.areaT[cL], area_R = g.areaT[cR];
  double hL[NKM], hR[NKM], pL[NKM], pR[NKM], h_vel[NKM], F[NKM];
  double dz[2 * NKM + 2], pLz[2 * NKM + 2], pRz[2 * NKM + 2], Fz[2 * NKM + 2];
  RemapWork<NKM> W;
  for (int k = 0; k < nk; k++) {
    hL[k] = A.h[cL + hpl * k]; hR[k] = A.h[cR + hpl * k];
    pL[k] = A.t[cL + hpl * k]; pR[k] = A.t[cR + hpl * k];
    h_vel[k] = (hL[k] + hR[k] == 0.) ? 0. : 2. * (hL[k] * hR[k]) / (hL[k] + hR[k]);
  }
  for (int k = 0; k < km; k++) { dz[k] = A.dz[DIR][f + fpl * k]; Fz[k] = 0.0; }
  remapping_core_h<NKM>(W, A.scheme, A.extrap != 0, nk, hL, pL, km, dz, pLz, A.h_neglect);
  remapping_core_h<NKM>(W, A.scheme, A.extrap != 0, nk, hR, pR, km, dz, pRz, A.h_neglect);
  const double *khz = A.khz[DIR] + f;
  int k_bot_L, k_bot_R;      // boundary_k_range(SURFACE, ...) :609-647 on the HBD grid
  double zeta_bot;
  m6::boundary_k_range_surface(dz, 1, km, hbl_L, k_bot_L, zeta_bot);
  m6::boundary_k_range_surface(dz, 1, km, hbl_R, k_bot_R, zeta_bot);
  const int k_bot_min = min(k_bot_L, k_bot_R), k_bot_max = max(k_bot_L, k_bot_R);
  for (int k = k_bot_min; k >= 1; k--) {      // 1-based as in the reference
    Fz[k - 1] = -(dz[k - 1] * khz[fpl * (k - 1)]) * (pRz[k - 1] - pLz[k - 1]);
    if (A.limiter_remap) Fz[k - 1] = flux_limiter(Fz[k - 1], area_L, area_R, pLz[k - 1], pRz[k - 1], dz[k - 1], dz[k - 1]);
  }
  if (A.linear && (k_bot_max - k_bot_min) > 1) {      // the linear decay at the base of hbl :781-796
    double htot = 0.0;
    for (int k = k_bot_min + 1; k <= k_bot_max; k++) htot = htot + dz[k - 1];
    const double a = -1.0 / htot;
    htot = 0.;
    for (int k = k_bot_min + 1; k <= k_bot_max; k++) {
      const double wgt = (a * (htot + (dz[k - 1] * 0.5))) + 1.0;
      Fz[k - 1] = -(dz[k - 1] * khz[fpl * (k - 1)]) * (pRz[k - 1] - pLz[k - 1]) * wgt;
      htot = htot + dz[k - 1];
      if (A.limiter_remap) Fz[k - 1] = flux_limiter(Fz[k - 1], area_L, area_R, pLz[k - 1], pRz[k - 1], dz[k - 1], dz[k - 1]);
    }
  }
  reintegrate_column(km, dz, Fz, nk, h_vel, F);
  for (int k = 0; k < nmax; k++) {
    double Fk = 0.0;
    if (k < nf) {      // the layers from nf on lie below htot_max (:818)
      Fk = F[k];
      if (A.limiter && Fk != 0.) Fk = flux_limiter(Fk, area_L, area_R, pL[k], pR[k], hL[k], hR[k]);
    }
    flx[f + fpl * k] = Fk;
  }
}

// What the diagnostic forms below take: where hbdxy_cont goes (the array, or scratch when only hbdxy_cont_2d is asked for) and hbdxy_conc
// (null: not asked for); the arrays of the face march
struct HBDMixOut { double *cont, *conc; double Idt; };
struct HBDFaceOut { double *a3, *a2; double Idt; };

// thread (i, j, k) over the compute domain.  D: nothing, or one HBDMixOut -- the form that also stores the tendency (:268-271) and its
// concentration form (:329-333), 0 on land (tendency(:,:,:) = 0.0, :232)
template <typename... D>
__global__ __launch_bounds__(256) void hbd_update_kernel(HBDArgs A, D... d) {
  constexpr bool DIAG = sizeof...(D) > 0;
  const m6::GridDev &g = A.g;
  const int i = g.isc + blockIdx.x * blockDim.x + threadIdx.x, j = g.jsc + blockIdx.y, k = blockIdx.z;
  if (i > g.iec) return;
  const long hpl = (long)g.nih * g.njh, n = g.h2(i, j) + hpl * k;
  double x = A.t[n];
  if (g.mask2dT[g.h2(i, j)] > 0.) {
    const long upl = face_plane(g, 0), vpl = face_plane(g, 1);
    const int I = i, J = j;
    const double uW = k < A.nflx_max[0] ? A.flx[0][g.u2(I - 1, j) + upl * k] : 0.0;
    const double uE = k < A.nflx_max[0] ? A.flx[0][g.u2(I, j) + upl * k] : 0.0;
    const double vS = k < A.nflx_max[1] ? A.flx[1][g.v2(i, J - 1) + vpl * k] : 0.0;
    const double vN = k < A.nflx_max[1] ? A.flx[1][g.v2(i, J) + vpl * k] : 0.0;
    x = x + (((uW - uE)) + ((vS - vN))) * g.IareaT[g.h2(i, j)] / (A.h[n] + g.H_subroundoff);
    if constexpr (DIAG) {
      const HBDMixOut &M = m6::nd_first(d...);
      const double td = ((uW - uE) + (vS - vN)) * g.IareaT[g.h2(i, j)] * M.Idt;
      if (M.cont) M.cont[n] = td;
      if (M.conc) M.conc[n] = td / (A.h[n] + g.H_subroundoff);
    }
  } else if constexpr (DIAG) {
    const HBDMixOut &M = m6::nd_first(d...);
    if (M.cont) M.cont[n] = 0.0;
    if (M.conc) M.conc[n] = 0.0;
  }
  if (A.cu > 0.0 && fabs(x) < A.cu) x = 0.0;
  A.t[n] = x;
}

// hbd_dfx / hbd_dfy (:292-293) and hbd_dfx_2d / hbd_dfy_2d (:294-308) of the tracer whose fluxes stand in A.flx: one thread a face of the
// compute range marches k, stores flx*Idt (0 from nflx_max on, where no flux is kept) and the running sum from 0.0 in layer order
template <int DIR>
__global__ __launch_bounds__(64) void hbd_face_diag_kernel(HBDArgs A, HBDFaceOut O) {
  const m6::GridDev &g = A.g;
  long f = 0, cL = 0, cR = 0;
  bool in_range;
  hbd_face<DIR>(g, in_range, f, cL, cR);
  if (!in_range) return;
  const long fpl = face_plane(g, DIR);
  const int nmax = A.nflx_max[DIR];
  double sum = 0.0;
  for (int k = 0; k < g.nk; k++) {
    const double v = (k < nmax ? A.flx[DIR][f + fpl * k] : 0.0) * O.Idt;
    if (O.a3) O.a3[f + fpl * k] = v;
    sum = sum + v;
  }
  if (O.a2) O.a2[f] = sum;
}

template <int NKM>
void launch_setup(const HBDArgs &A, int nbu, int nju, int nbv, int njv, hipStream_t s) {
  hipLaunchKernelGGL((hbd_setup_kernel<NKM, 0>), dim3(nbu, nju), dim3(64), 0, s, A);
  hipLaunchKernelGGL((hbd_setup_kernel<NKM, 1>), dim3(nbv, njv), dim3(64), 0, s, A);
}

template <int NKM>
void launch_flux(const HBDArgs &A, int nbu, int nju, int nbv, int njv, hipStream_t s) {
  hipLaunchKernelGGL((hbd_flux_kernel<NKM, 0>), dim3(nbu, nju), dim3(64), 0, s, A);
  hipLaunchKernelGGL((hbd_flux_kernel<NKM, 1>), dim3(nbv, njv), dim3(64), 0, s, A);
}

}  // namespace

namespace m6 {

bool hbd_scheme_provided(int scheme) {
  return scheme == MOM6HIP_REMAP_PCM || scheme == MOM6HIP_REMAP_PLM || scheme == MOM6HIP_REMAP_PPM_H4 || scheme == MOM6HIP_REMAP_PPM_IH4 ||
         scheme == MOM6HIP_REMAP_PPM_CW;
}

// USE_HORIZONTAL_BOUNDARY_DIFFUSION, MOM_tracer_hor_diff.F90:408-472: num_itts calls of hor_bnd_diffusion with Coef_x = I_numitts *
// khdt_x at every interface, each after a group pass of the tracers.
int hbd_branch(const HordiffCall &c, const mom6hip_hor_bnd_diffusion_cs_t *hbd, double KhTr_min, bool full_depth_khtr_min) {
  mom6hip_ctx_t *ctx = c.ctx;
  Stager &st = c.st;
  const std::vector<double *> &d_tr = c.d_tr;
  M6_REQUIRE(hbd->initialized, "hor_bnd_diffusion: the control structure is not initialised");
  M6_REQUIRE(!hbd->debug, "hor_bnd_diffusion: HBD_DEBUG is not provided by libmom6hip");
  // (with the records of mom6hip_tracer_hordiff_mix_diag the hbd_* diagnostics are those the records ask for)
  M6_REQUIRE(!hbd->diagnostics || c.mix, "hor_bnd_diffusion: the hbd_* diagnostics are not provided by libmom6hip");
  M6_REQUIRE(hbd_scheme_provided(hbd->remap_scheme), "hor_bnd_diffusion: HBD_REMAPPING_SCHEME %d is not provided by libmom6hip "
             "(PCM, PLM, PPM_H4, PPM_IH4 and PPM_CW are)", hbd->remap_scheme);
  M6_REQUIRE(c.h_ML != nullptr, "hor_bnd_diffusion requires that visc%%h_ML is associated.");
  const m6::GridDev g = ctx->g;
  M6_REQUIRE(g.mask2dT && g.mask2dCu && g.mask2dCv && g.areaT && g.IareaT, "hor_bnd_diffusion: mask2dT, mask2dCu, mask2dCv, areaT and IareaT are needed");
  M6_REQUIRE(g.nk >= 1 && g.nk <= 128, "hor_bnd_diffusion: 1 to 128 layers are supported");
  hipStream_t s = ctx->stream;
  const int ntr = (int)d_tr.size(), nk = g.nk;
  const size_t hpl = (size_t)g.nih * g.njh, upl = (size_t)(g.nih + 1) * g.njh, vpl = (size_t)g.nih * (g.njh + 1);
  HBDArgs A;
  A.g = g; A.h = c.h; A.khdt[0] = c.khdt_x; A.khdt[1] = c.khdt_y; A.I_numitts = c.I_numitts; A.h_neglect = g.H_subroundoff;
  A.linear = hbd->linear; A.limiter = hbd->limiter; A.limiter_remap = hbd->limiter_remap; A.extrap = hbd->boundary_extrap;
  A.scheme = hbd->remap_scheme; A.t = nullptr; A.cu = 0.0;
  A.ebt = c.ebt_struct; A.KhTr_min = KhTr_min; A.full_depth_khtr_min = full_depth_khtr_min ? 1 : 0;
  double *hbl = (double *)st.scratch(sizeof(double) * hpl);
  A.kmax[0] = (int *)st.scratch(sizeof(int) * upl); A.nflx[0] = (int *)st.scratch(sizeof(int) * upl);
  A.kmax[1] = (int *)st.scratch(sizeof(int) * vpl); A.nflx[1] = (int *)st.scratch(sizeof(int) * vpl);
  A.maxes = (int *)st.scratch(64);
  M6_REQUIRE(!st.failed() && hbl && A.kmax[0] && A.nflx[0] && A.kmax[1] && A.nflx[1] && A.maxes, "hor_bnd_diffusion: out of device memory");
  A.hbl = hbl;
  // hbl = visc%h_ML; pass_var(hbl, halo=1) (:217-222).  h and hbl do not change between the calls: the HBD grid is built once.
  M6_HIP(hipMemcpyAsync(hbl, c.h_ML, sizeof(double) * hpl, hipMemcpyDeviceToDevice, s));
  {
    double *f1[1] = {hbl}; int32_t p1[1] = {MOM6HIP_POS_H}, n1[1] = {1};
    if (int rc = m6::group_pass(ctx, f1, p1, n1, 1)) return rc;
  }
  M6_HIP(hipMemsetAsync(A.maxes, 0, 4 * sizeof(int), s));
  const int ni = g.iec - g.isc + 1, nj = g.jec - g.jsc + 1;
  const int nbu = (ni + 1 + 63) / 64, nbv = (ni + 63) / 64;
  hipLaunchKernelGGL(hbd_count_kernel<0>, dim3(nbu, nj), dim3(64), 0, s, A);
  hipLaunchKernelGGL(hbd_count_kernel<1>, dim3(nbv, nj + 1), dim3(64), 0, s, A);
  int mx[4] = {0, 0, 0, 0};
  M6_HIP(hipMemcpyAsync(mx, A.maxes, sizeof(mx), hipMemcpyDeviceToHost, s));
  M6_HIP(hipStreamSynchronize(s));
  for (int d = 0; d < 2; d++) {
    M6_REQUIRE(mx[d] <= 2 * nk + 2 && mx[2 + d] <= nk, "Houston, we've had a problem in hbd_grid (nk cannot be > CS%%hbd_nk)");
    A.nflx_max[d] = mx[2 + d];
    const size_t fpl = d == 0 ? upl : vpl;
    A.dz[d] = mx[d] ? (double *)st.scratch(sizeof(double) * fpl * mx[d]) : nullptr;
    A.khz[d] = mx[d] ? (double *)st.scratch(sizeof(double) * fpl * mx[d]) : nullptr;
    A.flx[d] = mx[2 + d] ? (double *)st.scratch(sizeof(double) * fpl * mx[2 + d]) : nullptr;
    M6_REQUIRE(!st.failed() && (!mx[d] || (A.dz[d] && A.khz[d])) && (!mx[2 + d] || A.flx[d]), "hor_bnd_diffusion: out of device memory");
  }
  const int nkm = nk <= 16 ? 16 : nk <= 80 ? 80 : 128;
  if (mx[0] + mx[1] > 0) {
    if (nkm == 16) launch_setup<16>(A, nbu, nj, nbv, nj + 1, s);
    else if (nkm == 80) launch_setup<80>(A, nbu, nj, nbv, nj + 1, s);
    else launch_setup<128>(A, nbu, nj, nbv, nj + 1, s);
  }
  M6_HIP(hipGetLastError());
  std::vector<double *> pf(d_tr);
  std::vector<int32_t> ppos(ntr, MOM6HIP_POS_H), pnk(ntr, nk);
  // the diagnostics hor_bnd_diffusion posts (:292-333): where only hbdxy_cont_2d is asked for, the tendency of a tracer goes to scratch
  const MixDiag *mix = c.mix;
  double *cont_scr = nullptr;
  if (mix) {
    bool cont_to_scratch = false;
    for (int m = 0; m < ntr; m++) cont_to_scratch = cont_to_scratch || (mix[m].a[MIX_HBDXY_CONT_2D] && !mix[m].a[MIX_HBDXY_CONT]);
    if (cont_to_scratch) {
      cont_scr = (double *)st.scratch(sizeof(double) * hpl * nk);
      M6_REQUIRE(!st.failed() && cont_scr, "hor_bnd_diffusion: out of device memory for the diagnostics");
    }
  }
  for (int itt = 1; itt <= c.num_itts; itt++) {
    if (int rc = m6::group_pass(ctx, pf.data(), ppos.data(), pnk.data(), ntr)) return rc;      // :412, and :466 for itt > 1
    (*c.halo_updates)++;
    for (int m = 0; m < ntr; m++) {
      A.t = d_tr[m]; A.cu = c.cu[m];
      if (A.nflx_max[0] + A.nflx_max[1] > 0) {
        if (nkm == 16) launch_flux<16>(A, nbu, nj, nbv, nj + 1, s);
        else if (nkm == 80) launch_flux<80>(A, nbu, nj, nbv, nj + 1, s);
        else launch_flux<128>(A, nbu, nj, nbv, nj + 1, s);
      }
      double *const *a = mix ? mix[m].a : nullptr;
      if (a && (a[MIX_HBD_DFX] || a[MIX_HBD_DFX_2D]))      // A.flx holds this tracer's fluxes until the next tracer's launch
        hipLaunchKernelGGL(hbd_face_diag_kernel<0>, dim3(nbu, nj), dim3(64), 0, s, A, HBDFaceOut{a[MIX_HBD_DFX], a[MIX_HBD_DFX_2D], c.Idt});
      if (a && (a[MIX_HBD_DFY] || a[MIX_HBD_DFY_2D]))
        hipLaunchKernelGGL(hbd_face_diag_kernel<1>, dim3(nbv, nj + 1), dim3(64), 0, s, A, HBDFaceOut{a[MIX_HBD_DFY], a[MIX_HBD_DFY_2D], c.Idt});
      if (a && (a[MIX_HBDXY_CONT] || a[MIX_HBDXY_CONT_2D] || a[MIX_HBDXY_CONC])) {
        HBDMixOut mo = {a[MIX_HBDXY_CONT] ? a[MIX_HBDXY_CONT] : a[MIX_HBDXY_CONT_2D] ? cont_scr : nullptr, a[MIX_HBDXY_CONC], c.Idt};
        hipLaunchKernelGGL(hbd_update_kernel<HBDMixOut>, dim3((ni + 255) / 256, nj, nk), dim3(256), 0, s, A, mo);
        if (a[MIX_HBDXY_CONT_2D]) {
          CellSumMarch sum2d; sum2d.g = g; sum2d.n = 1; sum2d.a3[0] = mo.cont; sum2d.a2[0] = a[MIX_HBDXY_CONT_2D];
          cell_sum_march(sum2d, s);
        }
      } else
        hipLaunchKernelGGL(hbd_update_kernel<>, dim3((ni + 255) / 256, nj, nk), dim3(256), 0, s, A);
    }
  }
  M6_HIP(hipGetLastError());
  return 0;
}

}  // namespace m6

extern "C" uint64_t mom6hip_abi_sizeof_hor_bnd_diffusion_cs(void) { return sizeof(mom6hip_hor_bnd_diffusion_cs_t); }
