// tracer_advect.hip -- advect_tracer / advect_x / advect_y (src/tracer/MOM_tracer_advect.F90:52-1087)
// as gfx950 stencil kernels.
//
// Design (DESIGN.md "advect_tracer"):
//  * Everything is updated IN PLACE, like the reference, so an extra iteration or an inactive
//    row/layer costs no copy traffic.  In-place is made race-free by the thread mapping:
//      - advect_x: one 64-lane wavefront owns one (j,k) row and sweeps it west->east in 64-cell
//        chunks.  A wave-private LDS tile keeps the pre-update values of the chunk plus a 3-cell halo
//        on both sides (the left halo is carried over from the previous chunk, the right halo is read
//        before anything to its east is written), so every stencil operand is the reference's
//        "T_tmp"/old hprev/old uhr.  West-face fluxes come from the neighbouring lane by a wavefront
//        shuffle.  No __syncthreads anywhere.
//      - advect_y: one lane owns one i column of a layer and marches south->north with the j stencil
//        in a register ring (rows J-1..J+3); a row is written only after every row the stencil needs
//        has been read by the same lane.  All loads/stores are i-contiguous (512 B per wave).
//  * Algorithmic traffic per pass = read+write of Tr(ntr), hprev and the remaining transport:
//    (ntr+2)*16 B per cell; unchanged values (land, inactive faces) are not written back.
//  * domore_u/domore_v/domore_k stay on the device; only domore_k (nk ints) is read back per
//    iteration for the exit test (the reference's sum_across_PEs at :305).
//  * Said once: the flux of a tracer through a face (face_slopes, face_flux), the cell's tracer (cell_tracer, underflows) and the
//    remaining transport (remaining_transport) serve the marching and the general kernels; with_group turns (tracers in the group,
//    scheme) into template arguments.  mom6hip_advect_tracer_obc is a sequence of phases on one AdvCall: adv_check, adv_stage_in,
//    adv_work_space, adv_registries, adv_setup; an iteration adv_group_pass, adv_sweep (adv_pass x and y), adv_count_remaining; adv_outputs.
#include <algorithm>
#include <array>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <type_traits>

#include "common.hpp"
#include "flux_diag_march.hpp"

namespace m6 { int halo_update_field(mom6hip_ctx_t *ctx, double *f, int pos, int nk); }      // (group_pass etc.: common.hpp)

namespace {

constexpr int MAXG = 4;      // tracers processed per kernel instance (register budget)
constexpr int XHALO = 3;     // i-halo of the advect_x tile (Colella-Woodward PPM needs 3)
constexpr int XTW = 64 + 2 * XHALO;

enum { PLM = MOM6HIP_ADV_PLM, H3 = MOM6HIP_ADV_PPM_H3, CW = MOM6HIP_ADV_PPM };

struct AdvArgs {
  m6::GridDev g;
  double *tr[MAXG];
  double cu[MAXG];           // conc_underflow
  double *hprev, *uhr, *vhr;
  int *domore_u;             // (jsd:jed, nk)
  int *domore_v_in;          // (jsd-1:jed, nk), state on entry
  int *domore_v_out;         // state on exit
  const int *domore_k;       // (nk)
  int is, ie, js, je;        // the reference's advect_x/advect_y range arguments
  int write_mass;            // 1: this tracer group also updates hprev / uhr|vhr / domore flags
  int any_cu;                // any conc_underflow > 0 in this group
};

// The flux diagnostics of a tracer group, handed to the DIAG instantiations of the marching kernels only (AdvNoDiag otherwise, so that the
// instantiations without diagnostics are what they were).  A null pointer: that tracer did not ask.
//   face[m]  scratch, face-shaped: the pass's flux of tracer m through every face it worked on, times Idt (zeroed before the pass)
//   axy[m]   Tr(m)%advection_xy, updated in place by the lane that owns the cell (:671-676, :1051-1054)
//   doi      scratch, h-shaped: do_i of the pass (zeroed before the pass: a cell outside its range counts as false)
struct AdvDiag {
  double *face[MAXG], *axy[MAXG];
  int *doi;
  double Idt;
};
struct AdvNoDiag {};
template <bool DIAG> using AdvDiagArg = std::conditional_t<DIAG, AdvDiag, AdvNoDiag>;

// Orders this wave's LDS traffic: the hardware executes one wave's LDS instructions in order, so
// all that is needed is to stop the compiler from moving loads/stores across this point.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// "changed" in the bit-pattern sense (so that -0.0 -> +0.0 is written back like the reference does)
__device__ __forceinline__ bool changed(double a, double b) {
  return __double_as_longlong(a) != __double_as_longlong(b);
}

__device__ __forceinline__ double max3(double a, double b, double c) { return fmax(fmax(a, b), c); }
__device__ __forceinline__ double min3(double a, double b, double c) { return fmin(fmin(a, b), c); }

// x / d for a constant d (6 or 3), bit-identical to the IEEE division the reference performs but
// without the ~13-slot v_div/v_rcp sequence: q = x*RN(1/d) is within 1 ulp, the FMA residual
// r = x - d*q is exact, and RN(q + r*RN(1/d)) is then the correctly rounded quotient (Markstein's
// correction step; checked against x/d on 4e8 random operands in tests/).  Zero keeps its sign and
// operands outside [2^-900, 2^900] (where the residual could under/overflow) take the real division.
template <int D>
__device__ __forceinline__ double div_const(double x) {
  constexpr double d = (double)D, c = 1.0 / (double)D;
  const double q = x * c;
  const double r = __fma_rn(-d, q, x);
  const double qq = __fma_rn(r, c, q);
  const double ax = fabs(x);
  const bool fast = (ax > 0x1p-900) && (ax < 0x1p900);
  double res = fast ? qq : x;
  if (__builtin_expect(!fast && ax != 0.0, 0)) res = x / d;
  return res;
}

// limited slope, MOM_tracer_advect.F90:427-431 / :809-813
__device__ __forceinline__ double plm_slope(double Tp, double Tc, double Tm, double mask) {
  double dMx = max3(Tp, Tc, Tm) - Tc;
  double dMn = Tc - min3(Tp, Tc, Tm);
  return mask * copysign(min3(0.5 * fabs(Tp - Tm), 2.0 * dMx, 2.0 * dMn), Tp - Tm);
}

// Flux limiting of the remaining transport through one face, :486-513 / :872-899.
//   r_c      remaining transport through this face (positive towards +i / +j)
//   r_m, r_p remaining transport through the faces on the minus / plus side
//   h_m, h_p volumes of the cells on the minus / plus side;  a_m, a_p their areas
__device__ __forceinline__ void face_transport(double r_c, double r_m, double r_p, double h_m, double h_p,
                                               double a_m, double a_p, double min_h, double &hh,
                                               double &CFL, bool &limited) {
  const double tiny_h = DBL_MIN;
  limited = false;
  const bool none = (r_c == 0.0) || ((r_c < 0.0) && (h_p <= tiny_h)) || ((r_c > 0.0) && (h_m <= tiny_h));
  const bool neg = r_c < 0.0;
  hh = r_c;
  if (neg) {
    const double hup = h_p - a_p * min_h;
    const double hlos = fmax(0.0, r_p);
    if ((((hup - hlos) + r_c) < 0.0) && ((0.5 * hup + r_c) < 0.0)) {
      hh = min3(-0.5 * hup, -hup + hlos, 0.0);
      limited = true;
    }
  } else {
    const double hup = h_m - a_m * min_h;
    const double hlos = fmax(0.0, -r_m);
    if ((((hup - hlos) - r_c) < 0.0) && ((0.5 * hup - r_c) < 0.0)) {
      hh = max3(0.5 * hup, hup - hlos, 0.0);
      limited = true;
    }
  }
  // CFL = -uhh/hprev(i+1) or uhh/hprev(i): one division, the negation is exact
  const double q = (neg ? -hh : hh) / (neg ? h_p : h_m);
  if (none) { hh = 0.0; CFL = 0.0; limited = false; } else { CFL = q; }
}

// PPM edge values, CW84 monotonicity and the CFL-integrated flux, :526-556 / :911-941
template <int SCHEME>
__device__ __forceinline__ double ppm_flux(double Tp, double Tc, double Tm, double sm, double sc, double sp,
                                           double mask_prod, double hh, double CFL) {
  double aL, aR;
  if (SCHEME == H3) {
    aL = div_const<6>(5. * Tc + (2. * Tm - Tp));
    aL = fmax(fmin(Tc, Tm), aL); aL = fmin(fmax(Tc, Tm), aL);
    aR = div_const<6>(5. * Tc + (2. * Tp - Tm));
    aR = fmax(fmin(Tc, Tp), aR); aR = fmin(fmax(Tc, Tp), aR);
  } else {
    aL = 0.5 * ((Tm + Tc) + div_const<3>(sm - sc));
    aR = 0.5 * ((Tc + Tp) + div_const<3>(sc - sp));
  }
  double dA = aR - aL, mA = 0.5 * (aR + aL);
  const double dA2_6 = div_const<6>(dA * dA);
  if (mask_prod * (Tp - Tc) * (Tc - Tm) <= 0.) {
    aL = Tc; aR = Tc;
  } else if (dA * (Tc - mA) > dA2_6) {
    aL = 3. * Tc - 2. * aR;
  } else if (dA * (Tc - mA) < -dA2_6) {
    aR = 3. * Tc - 2. * aL;
  }
  double a6 = 6. * Tc - 3. * (aR + aL);
  if (hh >= 0.0)
    return hh * (aR - 0.5 * CFL * ((aR - aL) - a6 * (1. - 2. / 3. * CFL)));
  else
    return hh * (aL + 0.5 * CFL * ((aR - aL) + a6 * (1. - 2. / 3. * CFL)));
}

// The slopes the flux of one face needs, about its upwind cell c: PLM its own, CW84 those of c-1, c, c+1, H3 none.
// T?? are the five cells c-2 .. c+2, mk_? the mask products of the two faces of c-1, c, c+1.  The outer two cells come by reference:
// advect_x has them in LDS, and they are read where CW uses them, not before the call (and not at all by PLM and H3).
template <int SCHEME>
__device__ __forceinline__ void face_slopes(const double &Tmm, double Tm, double Tc, double Tp, const double &Tpp, double mk_m, double mk_c,
                                            double mk_p, double &sm, double &sc, double &sp) {
  sm = 0.; sc = 0.; sp = 0.;
  if (SCHEME == CW) sm = plm_slope(Tc, Tm, Tmm, mk_m);
  if (SCHEME != H3) sc = plm_slope(Tp, Tc, Tm, mk_c);
  if (SCHEME == CW) sp = plm_slope(Tpp, Tp, Tc, mk_p);
}

// The flux of one tracer through one face from the upwind cell's values and slopes, :515-556 / :901-941
template <int SCHEME>
__device__ __forceinline__ double face_flux(double Tp, double Tc, double Tm, double sm, double sc, double sp, double mk_c,
                                            double hh, double CFL) {
  if (SCHEME == PLM) {
    if (hh >= 0.0) return hh * (Tc + 0.5 * sc * (1. - CFL));
    else           return hh * (Tc - 0.5 * sc * (1. - CFL));
  }
  return ppm_flux<SCHEME>(Tp, Tc, Tm, sm, sc, sp, mk_c, hh, CFL);
}

// What is left of the transport through a face, :632-635 / :1021-1024
__device__ __forceinline__ double remaining_transport(double x, double hh, double neglect) {
  double r = x - hh;
  if (fabs(r) < neglect) r = 0.0;
  return r;
}

// The tracer of a cell after the pass, :649-662 / :1040-1059.  `upd` is the caller's own guard: advect_x and the general
// kernel pass do_i && Ihnew > 0, advect_y passes do_i, as the reference does.
__device__ __forceinline__ double cell_tracer(bool upd, double t_old, double hlst, double fl_p, double fl_m, double Ihnew) {
  double t_new = t_old;
  if (upd) t_new = (t_old * hlst - (fl_p - fl_m)) * Ihnew;
  return t_new;
}

// The user-controlled underflow, :683-687 / :1062-1066
__device__ __forceinline__ bool underflows(double t, double cu) { return cu > 0.0 && fabs(t) < cu; }

// New cell volume and the factors of the tracer update, :637-648 (x) / :1030-1039 (y).
template <bool CLAMP0>
__device__ __forceinline__ bool cell_volume(double hh_p, double hh_m, double h_old, double areaT,
                                            double h_neglect, double &h_new, double &hlst, double &Ihnew) {
  // returns do_i
  if ((hh_p != 0.0) || (hh_m != 0.0)) {
    hlst = h_old;
    h_new = h_old - (hh_p - hh_m);
    if (CLAMP0) h_new = fmax(h_new, 0.0);
    const double hmin = h_neglect * areaT;
    const bool thin = h_new < hmin;
    const double inv = 1.0 / (thin ? hmin : h_new);
    if (h_new <= 0.0) { Ihnew = 0.0; return false; }
    if (thin) hlst = hlst + (hmin - h_new);
    Ihnew = inv;
    return true;
  }
  h_new = h_old; hlst = h_old; Ihnew = 0.0;
  return false;
}

// ---------------------------------------------------------------------------------------------
// setup: uhr, vhr, hprev   (:152-178)
__global__ __launch_bounds__(256) void adv_setup_kernel(m6::GridDev g, const double *__restrict__ h_end,
                                                        const double *__restrict__ uhtr,
                                                        const double *__restrict__ vhtr,
                                                        const double *__restrict__ vol_prev,
                                                        double *__restrict__ hprev, double *__restrict__ uhr,
                                                        double *__restrict__ vhr) {
  // thread <-> (I, J) over the q-point extent (isd-1:ied, jsd-1:jed), which covers every array
  const int I = g.isd - 1 + blockIdx.x * blockDim.x + threadIdx.x;
  const int J = g.jsd - 1 + blockIdx.y;
  const int k = blockIdx.z;
  if (I > g.ied) return;
  const bool in_i = (I >= g.isc && I <= g.iec), in_j = (J >= g.jsc && J <= g.jec);
  if (J >= g.jsd) {   // u-point (I, j=J)
    double v = 0.0;
    if (in_j && I >= g.isc - 1 && I <= g.iec) v = uhtr[g.u3(I, J, k)];
    uhr[g.u3(I, J, k)] = v;
  }
  if (I >= g.isd) {   // v-point (i=I, J)
    double v = 0.0;
    if (in_i && J >= g.jsc - 1 && J <= g.jec) v = vhtr[g.v3(I, J, k)];
    vhr[g.v3(I, J, k)] = v;
  }
  if (I >= g.isd && J >= g.jsd) {   // h-point
    double hp = 0.0;
    if (in_i && in_j) {
      if (vol_prev) {
        hp = vol_prev[g.h3(I, J, k)];
      } else {
        const double aT = g.areaT[g.h2(I, J)], he = h_end[g.h3(I, J, k)];
        hp = fmax(0.0, aT * he + ((uhtr[g.u3(I, J, k)] - uhtr[g.u3(I - 1, J, k)]) +
                                  (vhtr[g.v3(I, J, k)] - vhtr[g.v3(I, J - 1, k)])));
        hp = hp + fmax(0.0, 1.0e-13 * hp - aT * he);
      }
    }
    hprev[g.h3(I, J, k)] = hp;
  }
}

// domore_u / domore_v re-evaluation, :215-225.  One block per (row, k).
struct ScanArgs {
  m6::GridDev g;
  const double *uhr, *vhr;
  int *domore_u, *domore_v;
  const int *domore_k;
  int ju0, ju1, iu0, iu1;   // u rows j and the I range scanned
  int jv0, jv1, iv0, iv1;   // v rows J and the i range scanned
};

__global__ __launch_bounds__(256) void adv_scan_kernel(ScanArgs a) {
  const m6::GridDev &g = a.g;
  const int k = blockIdx.y;
  if (a.domore_k[k] <= 0) return;
  const int r = blockIdx.x;            // row index over (jsd-1 : jed)
  // u row j = jsd-1+r
  {
    const int j = g.jsd - 1 + r;
    if (j >= a.ju0 && j <= a.ju1 && j >= g.jsd) {
      int *flag = &a.domore_u[(j - g.jsd) + g.njh * k];
      if (!*flag) {
        for (int I0 = a.iu0; I0 <= a.iu1; I0 += blockDim.x) {
          const int I = I0 + threadIdx.x;
          int nz = (I <= a.iu1) && (a.uhr[g.u3(I, j, k)] != 0.0);
          if (__syncthreads_or(nz)) { if (threadIdx.x == 0) *flag = 1; break; }
        }
      }
    }
  }
  {
    const int J = g.jsd - 1 + r;
    if (J >= a.jv0 && J <= a.jv1) {
      int *flag = &a.domore_v[(J - g.jsd + 1) + (g.njh + 1) * k];
      if (!*flag) {
        for (int i0 = a.iv0; i0 <= a.iv1; i0 += blockDim.x) {
          const int i = i0 + threadIdx.x;
          int nz = (i <= a.iv1) && (a.vhr[g.v3(i, J, k)] != 0.0);
          if (__syncthreads_or(nz)) { if (threadIdx.x == 0) *flag = 1; break; }
        }
      }
    }
  }
}

// domore_k(k) = any(domore_u(ju0:ju1,k)) .or. any(domore_v(jv0:jv1,k)), only where domore_k(k) > 0
// (:229-231, :265-267, :287-289).  One wave per k.
__global__ void adv_domore_k_kernel(m6::GridDev g, const int *domore_u, const int *domore_v, int *domore_k,
                                    int ju0, int ju1, int jv0, int jv1) {
  const int k = blockIdx.x;
  if (domore_k[k] <= 0) return;
  int any = 0;
  for (int j = ju0 + threadIdx.x; j <= ju1; j += blockDim.x) any |= domore_u[(j - g.jsd) + g.njh * k];
  for (int J = jv0 + threadIdx.x; J <= jv1; J += blockDim.x) any |= domore_v[(J - g.jsd + 1) + (g.njh + 1) * k];
  any = __syncthreads_or(any);
  if (threadIdx.x == 0) domore_k[k] = any ? 1 : 0;
}

// domore_v_out = domore_v_in, except that rows advect_y is about to process are cleared (:869).
__global__ void adv_vflags_prep_kernel(m6::GridDev g, const int *in, int *out, const int *domore_k, int js, int je) {
  const int n = (g.njh + 1) * g.nk;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
    const int k = t / (g.njh + 1);
    const int J = g.jsd - 1 + (t - k * (g.njh + 1));
    int v = in[t];
    if (domore_k[k] > 0 && J >= js - 1 && J <= je) v = 0;
    out[t] = v;
  }
}

// ---------------------------------------------------------------------------------------------
// advect_x: one wavefront per (j,k) row.
template <int NT, int SCHEME, bool DIAG = false>
__global__ __launch_bounds__(256) void adv_x_kernel(AdvArgs p, AdvDiagArg<DIAG> d) {
  const m6::GridDev &g = p.g;
  __shared__ double s_T[4][NT][XTW];
  __shared__ double s_h[4][XTW];
  __shared__ double s_u[4][XTW];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int k = blockIdx.y;
  const int j = p.js + blockIdx.x * 4 + wave;
  if (j > p.je) return;
  if (p.domore_k[k] <= 0) return;
  int *flag = &p.domore_u[(j - g.jsd) + g.njh * k];
  const bool active = (*flag != 0);
  if (!active && !p.any_cu) return;

  const double min_h = 0.1 * g.Angstrom_H;
  const double h_neglect = g.H_subroundoff;
  const long rowH = g.h3(g.isd, j, k);          // offset of (isd, j, k) in h-point arrays
  const long rowU = g.u3(g.isd, j, k);          // offset of face I = isd
  const long row2H = g.h2(g.isd, j), row2U = g.u2(g.isd, j);

  if (!active) {
    // only the user-controlled underflow applies to this row (:683-687)
    for (int i = p.is + lane; i <= p.ie; i += 64) {
#pragma unroll
      for (int m = 0; m < NT; m++) if (p.cu[m] > 0.0) {
        const double t = p.tr[m][rowH + (i - g.isd)];
        if (underflows(t, p.cu[m]) && changed(t, 0.0)) p.tr[m][rowH + (i - g.isd)] = 0.0;
      }
    }
    return;
  }

  double(*sT)[XTW] = s_T[wave];
  double *sh = s_h[wave], *su = s_u[wave];

  // chunks are aligned to the start of the array row
  const int c0 = (p.is - 1 - g.isd) >> 6, c1 = (p.ie - g.isd) >> 6;
  auto ldH = [&](const double *a, int i) -> double { return (i >= g.isd && i <= g.ied) ? a[rowH + (i - g.isd)] : 0.0; };
  auto ldU = [&](const double *a, int I) -> double { return (I >= g.isd - 1 && I <= g.ied) ? a[rowU + (I - g.isd)] : 0.0; };

  // first tile: cells i0-XHALO .. i0+63+XHALO
  {
    const int i0 = g.isd + 64 * c0;
    for (int q = lane; q < XTW; q += 64) {
      const int i = i0 - XHALO + q;
#pragma unroll
      for (int m = 0; m < NT; m++) sT[m][q] = ldH(p.tr[m], i);
      sh[q] = ldH(p.hprev, i);
      su[q] = ldU(p.uhr, i);
    }
  }
  double hh_carry = 0.0, fl_carry[NT];
#pragma unroll
  for (int m = 0; m < NT; m++) fl_carry[m] = 0.0;
  bool any_limited = false;

  for (int c = c0; c <= c1; c++) {
    const int i0 = g.isd + 64 * c;
    const int i = i0 + lane;                 // this lane's cell, and its east face I = i
    const int P = XHALO + lane;
    // prefetch the part of the next tile that is not already in LDS: cells i0+64+XHALO+lane
    double nT[NT], nh = 0.0, nu = 0.0;
    const bool more = (c < c1);
    if (more) {
      const int in = i0 + 64 + XHALO + lane;
#pragma unroll
      for (int m = 0; m < NT; m++) nT[m] = ldH(p.tr[m], in);
      nh = ldH(p.hprev, in);
      nu = ldU(p.uhr, in);
    }
    wave_sync();

    const bool face_ok = (i >= p.is - 1 && i <= p.ie);
    const bool cell_ok = (i >= p.is && i <= p.ie);
    double hh = 0.0, CFL = 0.0, flux[NT];
#pragma unroll
    for (int m = 0; m < NT; m++) flux[m] = 0.0;
    const double u_c = su[P];
    const double h_c = sh[P];
    double aT_c = 0.0;
    if (face_ok) {
      aT_c = g.areaT[row2H + (i - g.isd)];
      const double aT_e = g.areaT[row2H + (i + 1 - g.isd)];
      bool lim;
      face_transport(u_c, su[P - 1], su[P + 1], h_c, sh[P + 1], aT_c, aT_e, min_h, hh, CFL, lim);
      any_limited |= lim;
      const int up = (hh >= 0.0) ? 0 : 1;        // i_up = i + up
      const int Pu = P + up;
      const double mk_c = g.mask2dCu[row2U + (i + up - g.isd)] * g.mask2dCu[row2U + (i + up - 1 - g.isd)];
      double mk_m = 0.0, mk_p = 0.0;
      if (SCHEME == CW) {
        mk_m = g.mask2dCu[row2U + (i + up - 1 - g.isd)] * g.mask2dCu[row2U + (i + up - 2 - g.isd)];
        mk_p = g.mask2dCu[row2U + (i + up + 1 - g.isd)] * g.mask2dCu[row2U + (i + up - g.isd)];
      }
#pragma unroll
      for (int m = 0; m < NT; m++) {
        const double Tp = sT[m][Pu + 1], Tc = sT[m][Pu], Tm = sT[m][Pu - 1];
        double sm, sc, sp;
        face_slopes<SCHEME>(sT[m][Pu - 2], Tm, Tc, Tp, sT[m][Pu + 2], mk_m, mk_c, mk_p, sm, sc, sp);
        flux[m] = face_flux<SCHEME>(Tp, Tc, Tm, sm, sc, sp, mk_c, hh, CFL);
      }
      if constexpr (DIAG) {      // flux_x(I,j,m)*Idt of :665-667 / :694-696; flux_diag_march_kernel (adv_diag_apply) adds it where do_i allows
#pragma unroll
        for (int m = 0; m < NT; m++) if (d.face[m]) d.face[m][rowU + (i - g.isd)] = flux[m] * d.Idt;
      }
    }
    // west-face values from the neighbouring lane (lane 0: carried from the previous chunk)
    double hh_w = __shfl_up(hh, 1);
    if (lane == 0) hh_w = hh_carry;
    double fl_w[NT];
#pragma unroll
    for (int m = 0; m < NT; m++) {
      fl_w[m] = __shfl_up(flux[m], 1);
      if (lane == 0) fl_w[m] = fl_carry[m];
    }
    hh_carry = __shfl(hh, 63);
#pragma unroll
    for (int m = 0; m < NT; m++) fl_carry[m] = __shfl(flux[m], 63);

    // remaining transport, :632-635
    if (face_ok && p.write_mass) {
      const double u_new = remaining_transport(u_c, hh, g.uh_neglect[row2U + (i - g.isd)]);
      if (changed(u_new, u_c)) p.uhr[rowU + (i - g.isd)] = u_new;
    }
    // cell volume and tracers, :636-662, and underflow :683-687
    if (cell_ok) {
      double h_new, hlst, Ihnew;
      const bool do_i = cell_volume<false>(hh, hh_w, h_c, aT_c, h_neglect, h_new, hlst, Ihnew);
      if (p.write_mass && changed(h_new, h_c)) p.hprev[rowH + (i - g.isd)] = h_new;
#pragma unroll
      for (int m = 0; m < NT; m++) {
        const double t_old = sT[m][P];
        double t_new = cell_tracer(do_i && Ihnew > 0.0, t_old, hlst, flux[m], fl_w[m], Ihnew);
        if (underflows(t_new, p.cu[m])) t_new = 0.0;
        if (changed(t_new, t_old)) p.tr[m][rowH + (i - g.isd)] = t_new;
      }
      if constexpr (DIAG) {
        if (d.doi) d.doi[rowH + (i - g.isd)] = do_i ? 1 : 0;
        if (do_i) {      // :671-676
          const double IaT = g.IareaT[row2H + (i - g.isd)];
#pragma unroll
          for (int m = 0; m < NT; m++) if (d.axy[m]) {
            double *a = &d.axy[m][rowH + (i - g.isd)];
            *a = *a - ((flux[m] - fl_w[m]) * d.Idt) * IaT;
          }
        }
      }
    }
    wave_sync();
    // slide the tile east by 64 cells
    if (more) {
      double kT[NT], kh = 0.0, ku = 0.0;
      if (lane < 2 * XHALO) {
#pragma unroll
        for (int m = 0; m < NT; m++) kT[m] = sT[m][64 + lane];
        kh = sh[64 + lane]; ku = su[64 + lane];
      }
      wave_sync();
      if (lane < 2 * XHALO) {
#pragma unroll
        for (int m = 0; m < NT; m++) sT[m][lane] = kT[m];
        sh[lane] = kh; su[lane] = ku;
      }
#pragma unroll
      for (int m = 0; m < NT; m++) sT[m][2 * XHALO + lane] = nT[m];
      sh[2 * XHALO + lane] = nh; su[2 * XHALO + lane] = nu;
    }
  }
  if (p.write_mass) {
    const int lim = __any(any_limited ? 1 : 0);
    if (lane == 0) *flag = lim ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------------------------
// advect_y: one lane per (i,k) column.  The J range [js-1, je] of a 64-column strip is cut into
// `nseg` segments, one per wavefront of the block (occupancy: a single marching wave per strip leaves
// most of the chip idle).  In-place safety across segments: before the block's only barrier every wave
// has (a) filled its register ring with the rows at and below its first face and (b) copied the rows
// just above its last face -- which the next wave will overwrite early in its own march -- into LDS;
// after the barrier a wave reads global memory only inside its own segment.  Each wave starts with one
// face-only step at J = Ja-1 (recomputing the flux its southern neighbour also computes) so that no
// flux has to cross a wave boundary.
constexpr int YSEG_MAX = 8;      // the waves a block may have: sizes the kernel's LDS and its launch bounds
constexpr int YSEG = 4;          // the waves a block is given: measured best on MI355X (8: one block per CU; 1-2: too few waves)

template <int NT, int SCHEME, bool DIAG = false>
#ifndef ADVY_OCC
#define ADVY_OCC 2      // waves per SIMD the register allocation aims at (tools/build_variant.sh for experiments)
#endif
__global__ __launch_bounds__(64 * YSEG_MAX, ADVY_OCC) void adv_y_kernel(AdvArgs p, int seglen, AdvDiagArg<DIAG> d) {
  const m6::GridDev &g = p.g;
  constexpr int NHR = (SCHEME == CW) ? 3 : 2;        // foreign T rows needed above the segment's last face
  __shared__ double s_halo[YSEG_MAX][NHR * NT + 2][64];
  const int seg = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = p.is + blockIdx.x * 64 + lane;
  const int k = blockIdx.y;
  if (p.domore_k[k] <= 0) return;                    // block-uniform
  const bool lane_ok = (i <= p.ie);
  const int ii = lane_ok ? i : p.ie;                 // idle lanes shadow a valid column, never store
  const double min_h = 0.1 * g.Angstrom_H;
  const double h_neglect = g.H_subroundoff;
  const long colH = g.h3(ii, g.jsd, k), colV = g.v3(ii, g.jsd, k);
  const long col2H = g.h2(ii, g.jsd), col2V = g.v2(ii, g.jsd);
  const int sH = g.nih;                              // j stride of h- and v-point arrays
  auto gH = [&](const double *a, int j) -> double { return (j >= g.jsd && j <= g.jed) ? a[colH + (long)sH * (j - g.jsd)] : 0.0; };
  auto gV = [&](const double *a, int J) -> double { return (J >= g.jsd - 1 && J <= g.jed) ? a[colV + (long)sH * (J - g.jsd)] : 0.0; };
  auto ldA = [&](int j) -> double { return (j >= g.jsd && j <= g.jed) ? g.areaT[col2H + (long)sH * (j - g.jsd)] : 0.0; };
  auto ldM = [&](int J) -> double { return (J >= g.jsd - 1 && J <= g.jed) ? g.mask2dCv[col2V + (long)sH * (J - g.jsd)] : 0.0; };
  const int *dv_in = p.domore_v_in + (long)(g.njh + 1) * k - (g.jsd - 1);
  int *dv_out = p.domore_v_out + (long)(g.njh + 1) * k - (g.jsd - 1);
  // is face J one advect_y works on (:868)?  (uniform)
  const int J0 = p.js - 1, J1 = p.je;
  auto act_face = [&](int J) -> unsigned { return ((J >= J0 && J <= J1) && dv_in[J] != 0) ? 1u : 0u; };

  const int Ja = J0 + seg * seglen;                  // first face this wave owns
  const int Jb = (Ja + seglen - 1 < J1) ? Ja + seglen - 1 : J1;
  const bool have = (Ja <= J1);
  const int Js = (seg == 0) ? J0 : Ja - 1;           // first step (face-only when seg > 0)

  // Row-level sparsity for iterations >= 2: fb bit n = "face J-3+n is active" at step J (a wave-uniform
  // shift register, refilled one flag per step, two steps ahead of its first use).
  // T(r) feeds the fluxes of faces r-2..r+1 (CW: r-3..r+2); hprev(r) those of faces r-1, r; a cell is
  // updated only if one of its two faces is active, which the same masks cover.
  unsigned fb = 0;
  if (have) for (int n = 0; n < 16; n++) fb |= act_face(Js - 3 + n) << n;
  const unsigned all = p.any_cu ? 1u : 0u;           // the underflow test needs every cell
  auto need_T = [&](unsigned bits, int d) -> bool {  // row r = J + d
    const unsigned m = (SCHEME == CW) ? (0x3Fu << d) : (0xFu << (d + 1));
    return ((bits & m) | all) != 0;
  };
  auto need_h = [&](unsigned bits, int d) -> bool { return ((bits & (0x3u << (d + 4))) | all) != 0; };   // row r = J+2+d: faces r-1, r

  // ---- before the barrier: ring at step Js, and the rows above Jb into LDS ----
  double t0[NT], t1[NT], t2[NT], t3[NT], t4[NT], t5[NT];
  double h_c = 0., h_n = 0., v_s = 0., v_c = 0., v_n = 0., a_c = 0., a_n = 0.;
  double m_ss = 0., m_s = 0., m_c = 0., m_n = 0., m_nn = 0.;
#pragma unroll
  for (int m = 0; m < NT; m++) { t0[m] = t1[m] = t2[m] = t3[m] = t4[m] = t5[m] = 0.0; }
  if (have) {
#pragma unroll
    for (int m = 0; m < NT; m++) {
      if (SCHEME == CW) t0[m] = gH(p.tr[m], Js - 2);
      t1[m] = gH(p.tr[m], Js - 1);
      t2[m] = gH(p.tr[m], Js);
      t3[m] = gH(p.tr[m], Js + 1);
      t4[m] = gH(p.tr[m], Js + 2);
      if (SCHEME == CW) t5[m] = gH(p.tr[m], Js + 3);
    }
    h_c = gH(p.hprev, Js); h_n = gH(p.hprev, Js + 1);
    v_s = gV(p.vhr, Js - 1); v_c = gV(p.vhr, Js); v_n = gV(p.vhr, Js + 1);
    a_c = ldA(Js); a_n = ldA(Js + 1);
    if (SCHEME == CW) { m_ss = ldM(Js - 2); m_nn = ldM(Js + 2); }
    m_s = ldM(Js - 1); m_c = ldM(Js); m_n = ldM(Js + 1);
    double(*hl)[64] = s_halo[seg];
#pragma unroll
    for (int r = 0; r < NHR; r++) {
#pragma unroll
      for (int m = 0; m < NT; m++) hl[r * NT + m][lane] = gH(p.tr[m], Jb + 1 + r);
    }
    hl[NHR * NT][lane] = gH(p.hprev, Jb + 1);
    hl[NHR * NT + 1][lane] = gV(p.vhr, Jb + 1);
  }
  __syncthreads();
  if (!have) return;
  const double(*hl)[64] = s_halo[seg];

  double hh_prev = 0.0, fl_prev[NT];
#pragma unroll
  for (int m = 0; m < NT; m++) fl_prev[m] = 0.0;
  constexpr int DT_ = (SCHEME == CW) ? 4 : 3;        // the T row entering the ring is J + DT_
  unsigned pend = act_face(Js + 13);

  // One step of the march.  TAIL = the new rows may lie above Jb and then come from LDS.
  auto step = [&](const int J, auto tail_tag) __attribute__((always_inline)) {
    constexpr bool TAIL = decltype(tail_tag)::value;
    const int j = J;
    const bool own = (J >= Ja);                  // false only on the face-only first step of seg > 0
    // issue the loads of the rows that enter the rings at the next step
    double nt[NT], nh, nv;
    const int rT = J + DT_;
    if (!TAIL) {
      const bool nT = need_T(fb, DT_);
#pragma unroll
      for (int m = 0; m < NT; m++) nt[m] = nT ? p.tr[m][colH + (long)sH * (rT - g.jsd)] : 0.0;
      nh = need_h(fb, 0) ? p.hprev[colH + (long)sH * (J + 2 - g.jsd)] : 0.0;
      nv = p.vhr[colV + (long)sH * (J + 2 - g.jsd)];
    } else {
#pragma unroll
      for (int m = 0; m < NT; m++) {
        if (rT <= Jb) nt[m] = p.tr[m][colH + (long)sH * (rT - g.jsd)];
        else nt[m] = (rT <= Jb + NHR) ? hl[(rT - Jb - 1) * NT + m][lane] : 0.0;
      }
      if (J + 2 <= Jb) { nh = p.hprev[colH + (long)sH * (J + 2 - g.jsd)]; nv = p.vhr[colV + (long)sH * (J + 2 - g.jsd)]; }
      else { nh = (J + 2 == Jb + 1) ? hl[NHR * NT][lane] : 0.0; nv = (J + 2 == Jb + 1) ? hl[NHR * NT + 1][lane] : 0.0; }
    }
    const double na = ldA(J + 2);
    const double nm = ldM((SCHEME == CW) ? J + 3 : J + 2);
    const unsigned pend_next = act_face(J + 14);

    const bool act = (fb >> 3) & 1u;
    double hh = 0.0, CFL = 0.0, flux[NT];
#pragma unroll
    for (int m = 0; m < NT; m++) flux[m] = 0.0;
    if (act) {
      bool lim;
      face_transport(v_c, v_s, v_n, h_c, h_n, a_c, a_n, min_h, hh, CFL, lim);
      if (own && p.write_mass && __any((lim && lane_ok) ? 1 : 0) && lane == 0) dv_out[J] = 1;
      const bool up = !(hh >= 0.0);              // j_up = j + up
      // mask2dCv(i,J_up)*mask2dCv(i,J_up-1)
      const double mk_c = up ? (m_n * m_c) : (m_c * m_s);
#pragma unroll
      for (int m = 0; m < NT; m++) {
        const double Tm = up ? t2[m] : t1[m], Tc = up ? t3[m] : t2[m], Tp = up ? t4[m] : t3[m];
        const double Tmm = up ? t1[m] : t0[m], Tpp = up ? t5[m] : t4[m];      // (these four are read by CW only)
        const double mk_m = up ? (m_c * m_s) : (m_s * m_ss);
        const double mk_p = up ? (m_nn * m_n) : (m_n * m_c);
        double sm, sc, sp;
        face_slopes<SCHEME>(Tmm, Tm, Tc, Tp, Tpp, mk_m, mk_c, mk_p, sm, sc, sp);
        flux[m] = face_flux<SCHEME>(Tp, Tc, Tm, sm, sc, sp, mk_c, hh, CFL);
      }
    }
    // remaining transport, :1021-1024 (every row J, active or not)
    if (own && p.write_mass && lane_ok) {
      const double v_new = remaining_transport(v_c, hh, g.vh_neglect[col2V + (long)sH * (J - g.jsd)]);
      if (changed(v_new, v_c)) p.vhr[colV + (long)sH * (J - g.jsd)] = v_new;
    }
    if constexpr (DIAG) {      // flux_y(i,m,J)*Idt of :1072-1074 / :1080-1082 (zero on a face that is not active)
      if (own && lane_ok) {
#pragma unroll
        for (int m = 0; m < NT; m++) if (d.face[m]) d.face[m][colV + (long)sH * (J - g.jsd)] = flux[m] * d.Idt;
      }
    }
    // cell j = J, :1028-1059, and underflow :1062-1066
    if (own && J >= p.js && lane_ok) {
      double h_new, hlst, Ihnew;
      const bool do_i = cell_volume<true>(hh, hh_prev, h_c, a_c, h_neglect, h_new, hlst, Ihnew);
      if (p.write_mass && changed(h_new, h_c)) p.hprev[colH + (long)sH * (j - g.jsd)] = h_new;
#pragma unroll
      for (int m = 0; m < NT; m++) {
        const double t_old = t2[m];
        double t_new = cell_tracer(do_i, t_old, hlst, flux[m], fl_prev[m], Ihnew);
        if (underflows(t_new, p.cu[m])) t_new = 0.0;
        if (changed(t_new, t_old)) p.tr[m][colH + (long)sH * (j - g.jsd)] = t_new;
      }
      if constexpr (DIAG) {
        if (d.doi) d.doi[colH + (long)sH * (j - g.jsd)] = do_i ? 1 : 0;
        if (do_i) {      // :1051-1054
          const double IaT = g.IareaT[col2H + (long)sH * (j - g.jsd)];
#pragma unroll
          for (int m = 0; m < NT; m++) if (d.axy[m]) {
            double *a = &d.axy[m][colH + (long)sH * (j - g.jsd)];
            *a = *a - ((flux[m] - fl_prev[m]) * d.Idt) * IaT;
          }
        }
      }
    }
    // advance the rings
    hh_prev = hh;
#pragma unroll
    for (int m = 0; m < NT; m++) {
      fl_prev[m] = flux[m];
      t0[m] = t1[m]; t1[m] = t2[m]; t2[m] = t3[m]; t3[m] = t4[m];
      if (SCHEME == CW) { t4[m] = t5[m]; t5[m] = nt[m]; } else { t4[m] = nt[m]; }
    }
    h_c = h_n; h_n = nh;
    v_s = v_c; v_c = v_n; v_n = nv;
    a_c = a_n; a_n = na;
    m_ss = m_s; m_s = m_c; m_c = m_n;
    if (SCHEME == CW) { m_n = m_nn; m_nn = nm; } else { m_n = nm; }
    fb = (fb >> 1) | (pend << 15);
    pend = pend_next;
  };

  // main part: every row that enters the rings lies inside the segment (and inside the array)
  int J = Js;
  const int Jmain = ((Jb - DT_ < g.jed - DT_) ? Jb - DT_ : g.jed - DT_);
  for (; J <= Jmain; J++) step(J, std::false_type{});
  for (; J <= Jb; J++) step(J, std::true_type{});
}

// The run-time pair (tracers in the group 1..MAXG, scheme) as compile-time constants: f(Int<NT>, Int<SCHEME>).
template <int N> using Int = std::integral_constant<int, N>;
template <class F>
void with_group(int n, int scheme, F &&f) {
  auto with_scheme = [&](auto nt) {
    if (scheme == PLM) f(nt, Int<PLM>{}); else if (scheme == H3) f(nt, Int<H3>{}); else f(nt, Int<CW>{});
  };
  switch (n) {
    case 1: with_scheme(Int<1>{}); break;
    case 2: with_scheme(Int<2>{}); break;
    case 3: with_scheme(Int<3>{}); break;
    default: with_scheme(Int<4>{}); break;
  }
}

// ---------------------------------------------------------------------------------------------
// The general form of advect_x / advect_y: two plain kernels a pass, a thread a face (the transport taken through the face and the fluxes
// of every tracer, :485-627 / :868-1014, into scratch) and a thread a cell (:632-687 / :1021-1066).  It is the path of an OBC whose
// segments carry tracer registries (segment%tr_Reg: a registered tracer takes its reservoir value or inflow concentration in the cell outside
// the segment :441-462 / :823-846, the slopes of the three cells about the segment's face are formed again, each with the masks of its own two
// faces (the loop index of :466 / :850 is the I / J of the mask expression: Fortran does not tell the cases apart) :463-473 / :847-856, an inflow carries the reservoir value with the whole remaining transport :580-627 / :965-1014); regional
// configurations are small, and the marching kernels above stay as they are.  MOM6HIP_ADV_GENERIC=1 takes this path without OBC (tests).
constexpr int MAXTR = 64;      // the tracers of a call (the context's staging buffers; GenTr)
struct GenTr { double *t[MAXTR]; double cu[MAXTR]; int ntr; };
struct GenSeg {      // a segment of the direction of the pass that has a tracer registry
  int plus;          // OBC_DIRECTION_E | N: the cell outside is the second cell of its faces
  int specified, A, c0, c1;      // the face index (IsdB | JsdB) and the range across it (jsd:jed | isd:ied)
  int a0, na, b0, nb;            // its own arrays: element (a, b, k) at (a - a0) + na * ((b - b0) + nb * k)
  int r0, ntseg;                 // its registry: regs[r0 .. r0 + ntseg)
};
struct GenReg { int m; const double *tres; double conc; };
struct GenArgs {
  m6::GridDev g;
  GenTr T;
  double *hprev, *xr;            // xr: uhr | vhr
  double *hh, *flux;             // scratch: the transport taken through every face in this pass; the fluxes, + fstride a tracer
  long fstride;
  int *dom_in, *dom_new;         // the rows' flags on entry; where a limited face flags its row for another pass
  const int *domore_k;
  const double *neglect;         // uh_neglect | vh_neglect
  int is, ie, js, je;
  int nseg; const GenSeg *segs; const GenReg *regs;
  int obc_any, obc_open;         // OBC%specified_?_BCs_exist_globally .or. OBC%open_?_BCs_exist_globally ; OBC%open_?_BCs_exist_globally
};

template <int DIR> __device__ __forceinline__ long gen_h2(const m6::GridDev &g, int n, int c) { return DIR ? g.h2(c, n) : g.h2(n, c); }
template <int DIR> __device__ __forceinline__ long gen_f2(const m6::GridDev &g, int n, int c) { return DIR ? g.v2(c, n) : g.u2(n, c); }

__device__ __forceinline__ double gen_seg_value(const GenSeg &s, const GenReg &r, int a, int b, int k) {
  if (!r.tres) return r.conc;
  return r.tres[(a - s.a0) + (long)s.na * ((b - s.b0) + (long)s.nb * k)];
}

template <int DIR, int SCHEME>
__global__ __launch_bounds__(256) void gen_flux_kernel(GenArgs p) {
  const m6::GridDev &g = p.g;
  const int tx = blockIdx.x * 256 + threadIdx.x, k = blockIdx.z;
  const int n = (DIR ? p.js - 1 + (int)blockIdx.y : p.is - 1 + tx);      // the face index along the direction
  const int c = (DIR ? p.is + tx : p.js + (int)blockIdx.y);             // the index across it
  if (DIR ? (c > p.ie) : (n > p.ie)) return;
  if (p.domore_k[k] <= 0) return;
  const long hpl = (long)g.nih * g.njh, fpl = DIR ? (long)g.nih * (g.njh + 1) : (long)(g.nih + 1) * g.njh;
  const long f2 = gen_f2<DIR>(g, n, c), f3 = f2 + fpl * k;
  const long fstep = DIR ? g.nih : 1;      // to the next face along the direction
  const int row = DIR ? (n - g.jsd + 1) + (g.njh + 1) * k : (c - g.jsd) + g.njh * k;
  const bool active = p.dom_in[row] != 0;
  if (!active) {
    if (DIR) { p.hh[f3] = 0.0; for (int m = 0; m < p.T.ntr; m++) p.flux[p.fstride * m + f3] = 0.0; }
    return;
  }
  const double min_h = 0.1 * g.Angstrom_H;
  const int nlo = DIR ? g.jsd : g.isd, nhi = DIR ? g.jed : g.ied;      // cells of the data domain along the direction
  const double *mask = DIR ? g.mask2dCv : g.mask2dCu;
  auto fmask = [&](int nn) { return mask[gen_f2<DIR>(g, nn, c)]; };
  // T_tmp of tracer m at the cell nn of this line
  auto Tt = [&](int m, int nn) -> double {
    double v = (nn >= nlo && nn <= nhi) ? p.T.t[m][gen_h2<DIR>(g, nn, c) + hpl * k] : 0.0;
    for (int q = 0; q < p.nseg; q++) {
      const GenSeg &s = p.segs[q];
      if (c < s.c0 || c > s.c1 || nn != (s.plus ? s.A + 1 : s.A)) continue;
      for (int r = s.r0; r < s.r0 + s.ntseg; r++)
        if (p.regs[r].m == m) v = DIR ? gen_seg_value(s, p.regs[r], c, s.A, k) : gen_seg_value(s, p.regs[r], s.A, c, k);
    }
    return v;
  };
  auto Traw = [&](int m, int nn) -> double { return (nn >= nlo && nn <= nhi) ? p.T.t[m][gen_h2<DIR>(g, nn, c) + hpl * k] : 0.0; };
  // the slopes are those of the tracer itself (:425-436), but for the three cells about a segment's face, formed again from T_tmp (:466-474)
  auto slope = [&](int m, int nn) -> double {
    for (int q = 0; q < p.nseg; q++) {
      const GenSeg &s = p.segs[q];
      if (c >= s.c0 && c <= s.c1 && nn >= s.A - 1 && nn <= s.A + 1)
        return plm_slope(Tt(m, nn + 1), Tt(m, nn), Tt(m, nn - 1), fmask(nn) * fmask(nn - 1));      // (:472, :854: Fortran's I is i -- the loop cell's masks)
    }
    return plm_slope(Traw(m, nn + 1), Traw(m, nn), Traw(m, nn - 1), fmask(nn) * fmask(nn - 1));
  };
  const long hm = gen_h2<DIR>(g, n, c), hp = gen_h2<DIR>(g, n + 1, c);
  double hh, CFL;
  bool lim;
  face_transport(p.xr[f3], p.xr[f3 - fstep], p.xr[f3 + fstep], p.hprev[hm + hpl * k], p.hprev[hp + hpl * k], g.areaT[hm], g.areaT[hp], min_h,
                 hh, CFL, lim);
  if (lim) atomicOr(&p.dom_new[row], 1);
  const int up = (hh >= 0.0) ? 0 : 1, cu = n + up;
  for (int m = 0; m < p.T.ntr; m++) {
    const double Tc = Tt(m, cu);
    double Tp = 0., Tm = 0., sm = 0., sc = 0., sp = 0.;
    if (SCHEME != PLM) { Tp = Tt(m, cu + 1); Tm = Tt(m, cu - 1); }
    if (SCHEME == CW) sm = slope(m, cu - 1);
    if (SCHEME != H3) sc = slope(m, cu);
    if (SCHEME == CW) sp = slope(m, cu + 1);
    const double fl = face_flux<SCHEME>(Tp, Tc, Tm, sm, sc, sp, fmask(cu) * fmask(cu - 1), hh, CFL);
    p.flux[p.fstride * m + f3] = fl;
  }
  // the inflows through the faces of the segments (two loops over the segments, as the reference)
  if (p.nseg > 0 && p.obc_any) {
    const double r = p.xr[f3];
    for (int pass = 0; pass < 2; pass++) {
      if (pass == 1 && !p.obc_open) break;
      for (int q = 0; q < p.nseg; q++) {
        const GenSeg &s = p.segs[q];
        if (n != s.A || c < s.c0 || c > s.c1) continue;
        bool inflow;
        if (pass == 0) {
          if (DIR && !s.specified) continue;      // (advect_y :969; advect_x takes every segment :583)
          inflow = ((r > 0.0) && !s.plus) || ((r < 0.0) && s.plus);
        } else {
          if (s.specified) continue;
          inflow = ((r > 0.0) && (g.mask2dT[hm] < 0.5)) || ((r < 0.0) && (g.mask2dT[hp] < 0.5));
        }
        if (!inflow) continue;
        hh = r;
        for (int t = s.r0; t < s.r0 + s.ntseg; t++)
          p.flux[p.fstride * p.regs[t].m + f3] = hh * (DIR ? gen_seg_value(s, p.regs[t], c, s.A, k) : gen_seg_value(s, p.regs[t], s.A, c, k));
      }
    }
  }
  p.hh[f3] = hh;
}

template <int DIR>
__global__ __launch_bounds__(256) void gen_update_kernel(GenArgs p) {
  const m6::GridDev &g = p.g;
  const int tx = blockIdx.x * 256 + threadIdx.x, k = blockIdx.z;
  const int n = (DIR ? p.js - 1 + (int)blockIdx.y : p.is - 1 + tx);
  const int c = (DIR ? p.is + tx : p.js + (int)blockIdx.y);
  if (DIR ? (c > p.ie) : (n > p.ie)) return;
  if (p.domore_k[k] <= 0) return;
  const long hpl = (long)g.nih * g.njh, fpl = DIR ? (long)g.nih * (g.njh + 1) : (long)(g.nih + 1) * g.njh;
  const long f2 = gen_f2<DIR>(g, n, c), f3 = f2 + fpl * k;
  const long fstep = DIR ? g.nih : 1;
  const bool active = DIR ? true : (p.dom_in[(c - g.jsd) + g.njh * k] != 0);
  const bool cell = n >= (DIR ? p.js : p.is);
  const long h2 = gen_h2<DIR>(g, n, c), h3 = h2 + hpl * k;
  if (active) {
    const double hh = p.hh[f3];
    p.xr[f3] = remaining_transport(p.xr[f3], hh, p.neglect[f2]);
    if (cell) {
      const double hh_m = p.hh[f3 - fstep], h_old = p.hprev[h3];
      double h_new, hlst, Ihnew;
      const bool do_i = DIR ? cell_volume<true>(hh, hh_m, h_old, g.areaT[h2], g.H_subroundoff, h_new, hlst, Ihnew)
                            : cell_volume<false>(hh, hh_m, h_old, g.areaT[h2], g.H_subroundoff, h_new, hlst, Ihnew);
      if (changed(h_new, h_old)) p.hprev[h3] = h_new;
      if (do_i && Ihnew > 0.0)
        for (int m = 0; m < p.T.ntr; m++) {
          const double t_old = p.T.t[m][h3];
          p.T.t[m][h3] = cell_tracer(true, t_old, hlst, p.flux[p.fstride * m + f3], p.flux[p.fstride * m + f3 - fstep], Ihnew);
        }
    }
  }
  if (cell)      // :683-687 / :1062-1066
    for (int m = 0; m < p.T.ntr; m++) if (p.T.cu[m] > 0.0) {
      const double t = p.T.t[m][h3];
      if (underflows(t, p.T.cu[m]) && changed(t, 0.0)) p.T.t[m][h3] = 0.0;
    }
}

// advect_x: the flags of the rows that were processed take what the pass found (:413, :497, :507)
__global__ void gen_xflags_kernel(m6::GridDev g, int *dom, const int *dom_new, const int *domore_k, int js, int je) {
  const int n = g.njh * g.nk;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
    const int k = t / g.njh, j = g.jsd + (t - k * g.njh);
    if (domore_k[k] > 0 && j >= js && j <= je && dom[t]) dom[t] = dom_new[t];
  }
}

struct Timer {
  hipEvent_t a = nullptr, b = nullptr;
  bool on = false;
  hipStream_t s;
  Timer(bool enable, hipStream_t st) : on(enable), s(st) {
    if (on) { (void)hipEventCreate(&a); (void)hipEventCreate(&b); }
  }
  ~Timer() { if (on) { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } }
  void start() { if (on) (void)hipEventRecord(a, s); }
  // returns ms; synchronises (timing mode only)
  double stop() {
    if (!on) return 0.0;
    (void)hipEventRecord(b, s); (void)hipEventSynchronize(b);
    float ms = 0.f; (void)hipEventElapsedTime(&ms, a, b);
    return ms;
  }
};

// What one advect_tracer call carries from phase to phase (the pattern of BtCall in barotropic.hip).
struct AdvCall {
  mom6hip_ctx_t *ctx; const mom6hip_tracer_advect_cs_t *cs; const mom6hip_obc_t *obc; hipStream_t s; m6::GridDev g;
  // the caller's arguments
  const double *h_end, *uhtr, *vhtr, *conc_underflow;
  double *const *tr; double *vol_prev, *uhr_out, *vhr_out;
  int ntr, memspace, update_vol_prev;
  // the switches and ranges of the call; bytes of an h-, u-, v-point array; elements of domore_u, domore_v
  int is, ie, js, je, nz, stencil, max_iter;
  bool x_first, generic;
  size_t bH, bU, bV, nfu, nfv;
  // device views of the caller's arrays; work space and flags
  const double *d_in[4];      // h_end, uhtr, vhtr, vol_prev (or null)
  std::vector<double *> d_tr;
  double *hprev, *uhr, *vhr;
  int *domore_u, *domore_v, *domore_v2, *domore_k;
  // the general path: the segments with a registry by direction, their registries, the scratch of a pass (hh, then the fluxes)
  std::vector<GenSeg> gsegs[2]; std::vector<GenReg> gregs;
  GenSeg *d_gsegs[2]; GenReg *d_gregs; double *gen_scratch; size_t fmax_el; int *gen_flags;
  // the flux diagnostics (null: none asked for): the caller's records; per tracer the device views of its five arrays (ad_x, ad_y, ad2d_x,
  // ad2d_y, advection_xy) and its slot of face scratch (-1: no face diagnostic); the scratch of a pass (the slots, then doi)
  const mom6hip_tracer_flux_diag_t *diag; double Idt;
  std::vector<std::array<double *, 5>> d_diag; std::vector<int> diag_slot;
  double *diag_face; int *diag_doi; size_t diag_scratch_bytes; int diag_nslots;
  // the iteration (:203): its number, the range still valid, what the statistics report
  int itt, isv, iev, jsv, jev, halo_updates, remaining;
  Timer *t_k; mom6hip_advect_timing_t tm;
};

// the checks of the arguments, then the stencil, the sweep order and the iteration limit (:126-150)
int adv_check(AdvCall &c, double dt, int x_first_in, int max_iter_in) {
  const mom6hip_tracer_advect_cs_t *cs = c.cs; const m6::GridDev &g = c.g; const int ntr = c.ntr;
  M6_REQUIRE(cs != nullptr, "advect_tracer: tracer_advect_init must be called before advect_tracer");
  M6_REQUIRE(c.h_end && c.uhtr && c.vhtr && c.tr, "advect_tracer: null field pointer");
  M6_REQUIRE(cs->scheme == PLM || cs->scheme == H3 || cs->scheme == CW,
             "MOM_tracer_advect: Unknown TRACER_ADVECTION_SCHEME = %d", cs->scheme);
  M6_REQUIRE(c.memspace == MOM6HIP_MEM_HOST || c.memspace == MOM6HIP_MEM_DEVICE, "advect_tracer: bad memspace");
  M6_REQUIRE(ntr <= MAXTR, "advect_tracer: at most 64 tracers are supported");
  M6_REQUIRE(dt > 0.0 && cs->dt > 0.0, "advect_tracer: dt must be positive");
  for (int m = 0; m < ntr; m++) M6_REQUIRE(c.tr[m] != nullptr, "advect_tracer: tracer %d is null", m);

  c.is = g.isc; c.ie = g.iec; c.js = g.jsc; c.je = g.jec; c.nz = g.nk;
  c.bH = (size_t)g.nh3() * 8; c.bU = (size_t)g.nu3() * 8; c.bV = (size_t)g.nv3() * 8;
  c.stencil = 2;
  if (cs->scheme != PLM && !cs->use_huynh_stencil_bug) c.stencil = 3;
  M6_REQUIRE(c.is - g.isd >= c.stencil && g.ied - c.ie >= c.stencil && c.js - g.jsd >= c.stencil && g.jed - c.je >= c.stencil,
             "advect_tracer: halo (%d) narrower than the advection stencil (%d)", c.is - g.isd, c.stencil);
  c.x_first = (c.ctx->host.first_direction % 2) == 0;
  c.max_iter = 2 * (int)ceil(dt / cs->dt) + 1;
  if (max_iter_in > 0) c.max_iter = max_iter_in;
  if (x_first_in >= 0) c.x_first = x_first_in != 0;
  return 0;
}

// device views of the caller's arrays
int adv_stage_in(AdvCall &c) {
  mom6hip_ctx_t *ctx = c.ctx; hipStream_t s = c.s;
  const double *src[4] = {c.h_end, c.uhtr, c.vhtr, c.vol_prev};
  const size_t bytes[4] = {c.bH, c.bU, c.bV, c.bH};
  for (int q = 0; q < 4; q++) c.d_in[q] = src[q];
  c.d_tr.assign(c.tr, c.tr + c.ntr);
  if (c.memspace != MOM6HIP_MEM_HOST) return 0;
  for (int q = 0; q < 4; q++) {
    if (!src[q]) continue;      // (vol_prev absent)
    if (ctx->stage[q].reserve(bytes[q])) return 1;
    M6_HIP(hipMemcpyAsync(ctx->stage[q].p, src[q], bytes[q], hipMemcpyHostToDevice, s));
    c.d_in[q] = (const double *)ctx->stage[q].p;
  }
  for (int m = 0; m < c.ntr; m++) {
    if (ctx->tr_stage[m].reserve(c.bH)) return 1;
    M6_HIP(hipMemcpyAsync(ctx->tr_stage[m].p, c.tr[m], c.bH, hipMemcpyHostToDevice, s));
    c.d_tr[m] = (double *)ctx->tr_stage[m].p;
  }
  return 0;
}

// hprev, uhr, vhr; domore_u, two copies of domore_v (advect_y reads one and writes the other) and domore_k = 1
int adv_work_space(AdvCall &c) {
  mom6hip_ctx_t *ctx = c.ctx; const int nz = c.nz;
  c.nfu = (size_t)c.g.njh * nz; c.nfv = (size_t)(c.g.njh + 1) * nz;
  if (ctx->hprev.reserve(c.bH) || ctx->uhr.reserve(c.bU) || ctx->vhr.reserve(c.bV) ||
      ctx->flags.reserve((c.nfu + 2 * c.nfv + nz) * sizeof(int)))
    return 1;
  c.hprev = (double *)ctx->hprev.p; c.uhr = (double *)ctx->uhr.p; c.vhr = (double *)ctx->vhr.p;
  c.domore_u = (int *)ctx->flags.p; c.domore_v = c.domore_u + c.nfu; c.domore_v2 = c.domore_v + c.nfv;
  c.domore_k = c.domore_v2 + c.nfv;
  M6_HIP(hipMemsetAsync(c.domore_u, 0, (c.nfu + 2 * c.nfv) * sizeof(int), c.s));
  for (int k = 0; k < nz; k++) ctx->h_domore_k[k] = 1;
  M6_HIP(hipMemcpyAsync(c.domore_k, ctx->h_domore_k, nz * sizeof(int), hipMemcpyHostToDevice, c.s));
  return 0;
}

// The general path is taken for the tracer registries of the segments (OBC%OBC_pe), or on request: the segments that have one as
// GenSeg by direction, their registered tracers as GenReg (a reservoir handed over as a host array is staged).
int adv_registries(AdvCall &c) {
  mom6hip_ctx_t *ctx = c.ctx; const mom6hip_obc_t *obc = c.obc; const m6::GridDev &g = c.g;
  c.generic = getenv("MOM6HIP_ADV_GENERIC") && atoi(getenv("MOM6HIP_ADV_GENERIC")) != 0;
  ctx->adv_obc_n = 0;      // (the staged reservoirs of this call: counted from zero whatever a refused call left behind)
  if (obc && obc->OBC_pe) {
    M6_REQUIRE(obc->number_of_segments == 0 || obc->segment, "advect_tracer: OBC%%segment is required");
    for (int n = 0; n < obc->number_of_segments; n++) {
      const mom6hip_obc_segment_t &S = obc->segment[n];
      if (!S.tr_Reg) continue;
      if (!(S.is_E_or_W || S.is_N_or_S)) continue;      // (not on this PE: read by neither advect_x nor advect_y)
      c.generic = true;
      const int d = S.is_N_or_S ? 1 : 0;
      GenSeg q;
      q.plus = (S.direction == MOM6HIP_OBC_DIRECTION_E || S.direction == MOM6HIP_OBC_DIRECTION_N) ? 1 : 0;
      q.specified = S.specified; q.A = d ? S.JsdB : S.IsdB; q.c0 = d ? S.isd : S.jsd; q.c1 = d ? S.ied : S.jed;
      q.a0 = d ? S.isd : S.IsdB; q.na = d ? (S.ied - S.isd + 1) : (S.IedB - S.IsdB + 1);
      q.b0 = d ? S.JsdB : S.jsd; q.nb = d ? (S.JedB - S.JsdB + 1) : (S.jed - S.jsd + 1);
      M6_REQUIRE(q.A >= (d ? g.jsd : g.isd) + 2 && q.A <= (d ? g.jed : g.ied) - 3 && q.c0 >= (d ? g.isd : g.jsd) && q.c1 <= (d ? g.ied : g.jed),
                 "advect_tracer: OBC segment %d lies outside the data domain", n + 1);
      q.r0 = (int)c.gregs.size(); q.ntseg = S.ntseg;
      for (int t = 0; t < S.ntseg; t++) {
        const mom6hip_obc_segment_tracer_t &R = S.tr_Reg[t];
        M6_REQUIRE(R.ntr_index >= 1 && R.ntr_index <= c.ntr, "advect_tracer: the registry of OBC segment %d names tracer %d of %d", n + 1, R.ntr_index, c.ntr);
        GenReg r; r.m = R.ntr_index - 1; r.conc = R.OBC_inflow_conc; r.tres = nullptr;
        if (R.tres) {
          const size_t bytes = (size_t)q.na * q.nb * c.nz * 8;
          if (c.memspace == MOM6HIP_MEM_HOST) {
            M6_REQUIRE(ctx->adv_obc_n < 64 && ctx->adv_obc[ctx->adv_obc_n].reserve(bytes) == 0, "advect_tracer: out of device memory for the tracer reservoirs");
            M6_HIP(hipMemcpyAsync(ctx->adv_obc[ctx->adv_obc_n].p, R.tres, bytes, hipMemcpyHostToDevice, c.s));
            r.tres = (const double *)ctx->adv_obc[ctx->adv_obc_n++].p;
          } else r.tres = R.tres;
        }
        c.gregs.push_back(r);
      }
      // the slopes about a segment are formed again with the tracer values of that moment: two segments with registries within three
      // cells of each other on a line would make the order of the reference's loop over the segments matter
      for (const GenSeg &o : c.gsegs[d])
        M6_REQUIRE(o.c1 < q.c0 || o.c0 > q.c1 || abs(o.A - q.A) > 3, "advect_tracer: OBC segments with tracer registries closer than four cells are not provided");
      c.gsegs[d].push_back(q);
    }
  }
  M6_REQUIRE(!c.generic || c.ntr <= MAXTR, "advect_tracer: at most %d tracers on the general path", MAXTR);
  // the general path's device memory: the scratch of a pass, the tables above, the flags gen_xflags_kernel reads
  hipStream_t s = c.s;
  c.fmax_el = (size_t)(g.nu3() > g.nv3() ? g.nu3() : g.nv3());
  if (!c.generic) return 0;
  const size_t bs0 = sizeof(GenSeg) * (c.gsegs[0].size() + 1), bs1 = sizeof(GenSeg) * (c.gsegs[1].size() + 1), br = sizeof(GenReg) * (c.gregs.size() + 1);
  if (c.ctx->adv_gen.reserve(bs0 + bs1 + br + 64 + c.nfu * sizeof(int) + c.fmax_el * 8 * ((size_t)c.ntr + 1))) return 1;
  char *q = (char *)c.ctx->adv_gen.p;
  c.gen_scratch = (double *)q; q += c.fmax_el * 8 * ((size_t)c.ntr + 1);
  c.d_gsegs[0] = (GenSeg *)q; q += bs0; c.d_gsegs[1] = (GenSeg *)q; q += bs1; c.d_gregs = (GenReg *)q; q += br;
  q = (char *)(((uintptr_t)q + 15) & ~(uintptr_t)15);
  c.gen_flags = (int *)q;
  for (int d = 0; d < 2; d++)
    if (!c.gsegs[d].empty()) M6_HIP(hipMemcpyAsync(c.d_gsegs[d], c.gsegs[d].data(), sizeof(GenSeg) * c.gsegs[d].size(), hipMemcpyHostToDevice, s));
  if (!c.gregs.empty()) M6_HIP(hipMemcpyAsync(c.d_gregs, c.gregs.data(), sizeof(GenReg) * c.gregs.size(), hipMemcpyHostToDevice, s));
  M6_HIP(hipStreamSynchronize(s));      // (the host vectors are read by the copies)
  return 0;
}

// The flux diagnostics asked for: device views of the arrays (staged copies with host arrays), zeroed whole (:193-197), and the scratch of
// a pass.  One block of the context holds the scratch and then the staged copies.
int adv_diag_setup(AdvCall &c) {
  if (!c.diag) return 0;
  const m6::GridDev &g = c.g; hipStream_t s = c.s;
  const size_t b2U = c.bU / c.nz, b2V = c.bV / c.nz, bytes[5] = {c.bU, c.bV, b2U, b2V, c.bH};
  c.d_diag.assign(c.ntr, std::array<double *, 5>{});
  c.diag_slot.assign(c.ntr, -1);
  bool any = false;
  size_t staged = 0;
  for (int m = 0; m < c.ntr; m++) {
    const mom6hip_tracer_flux_diag_t &D = c.diag[m];
    double *const src[5] = {D.ad_x, D.ad_y, D.ad2d_x, D.ad2d_y, D.advection_xy};
    for (int q = 0; q < 5; q++) if (src[q]) { any = true; staged += bytes[q]; }
    if (D.ad_x || D.ad_y || D.ad2d_x || D.ad2d_y) c.diag_slot[m] = c.diag_nslots++;
  }
  if (!any) { c.diag = nullptr; return 0; }
  M6_REQUIRE(!c.generic, "advect_tracer: the flux diagnostics (ad_x, ad_y, ad2d_x, ad2d_y, advection_xy) are not provided on the general "
                         "path (a tracer registry on an OBC segment, or MOM6HIP_ADV_GENERIC=1)");
  const bool host = (c.memspace == MOM6HIP_MEM_HOST);
  c.diag_scratch_bytes = (size_t)c.diag_nslots * c.fmax_el * 8 + (c.diag_nslots ? (size_t)g.nh3() * sizeof(int) : 0);
  if (c.ctx->adv_diag.reserve(c.diag_scratch_bytes + (host ? staged : 0) + 64)) return 1;
  char *q = (char *)c.ctx->adv_diag.p;
  c.diag_face = (double *)q; c.diag_doi = c.diag_nslots ? (int *)(q + (size_t)c.diag_nslots * c.fmax_el * 8) : nullptr;
  q += (c.diag_scratch_bytes + 7) & ~(size_t)7;
  for (int m = 0; m < c.ntr; m++) {
    const mom6hip_tracer_flux_diag_t &D = c.diag[m];
    double *const src[5] = {D.ad_x, D.ad_y, D.ad2d_x, D.ad2d_y, D.advection_xy};
    for (int n = 0; n < 5; n++) if (src[n]) {
      c.d_diag[m][n] = host ? (double *)q : src[n];
      if (host) q += bytes[n];
      M6_HIP(hipMemsetAsync(c.d_diag[m][n], 0, bytes[n], s));
    }
  }
  return 0;
}

// the diagnostics of tracer group grp for the pass in direction dir; false: none of its tracers asked for any
bool group_diag(const AdvCall &c, int grp, int dir, AdvDiag &d) {
  bool any = false;
  d.Idt = c.Idt; d.doi = nullptr;
  for (int m = 0; m < MAXG; m++) {
    const int t = grp * MAXG + m;
    d.face[m] = nullptr; d.axy[m] = nullptr;
    if (t >= c.ntr) continue;
    if (c.diag_slot[t] >= 0 && (c.d_diag[t][dir] || c.d_diag[t][2 + dir])) {
      d.face[m] = c.diag_face + (size_t)c.diag_slot[t] * c.fmax_el; d.doi = c.diag_doi; any = true;
    }
    if (c.d_diag[t][4]) { d.axy[m] = c.d_diag[t][4]; any = true; }
  }
  return any;
}

// after the marching kernels of a pass: the march over k (flux_diag_march.hpp) of every tracer that has a face diagnostic of this direction:
// ad_x | ad_y take the pass's flux*Idt where do_i holds on either side of the face (:665-667, :1070-1076), ad2d_x | ad2d_y the same in the
// order of k (:689-698, :1078-1084).  A row or layer the pass did not work on has zeros in the scratch and in doi.
int adv_diag_apply(AdvCall &c, int dir, int is, int ie, int js, int je) {
  m6::FluxDiagMarch a; a.g = c.g; a.doi = c.diag_doi; a.skip0 = a.skip1 = 0; a.zero = 0; a.is = is; a.ie = ie; a.js = js; a.je = je; a.n = 0;
  for (int t = 0; t < c.ntr; t++) {
    if (c.diag_slot[t] < 0 || !(c.d_diag[t][dir] || c.d_diag[t][2 + dir])) continue;
    a.face[a.n] = c.diag_face + (size_t)c.diag_slot[t] * c.fmax_el; a.a3[a.n] = c.d_diag[t][dir]; a.a2[a.n] = c.d_diag[t][2 + dir];
    if (++a.n == m6::FLUX_DIAG_MAXD) { m6::flux_diag_march(dir, a, c.s); a.n = 0; }
  }
  if (a.n) m6::flux_diag_march(dir, a, c.s);
  M6_HIP(hipGetLastError());
  return 0;
}

// uhr, vhr, hprev :152-178
int adv_setup(AdvCall &c) {
  const m6::GridDev &g = c.g;
  c.t_k->start();
  hipLaunchKernelGGL(adv_setup_kernel, dim3((g.nih + 1 + 255) / 256, g.njh + 1, c.nz), dim3(256), 0, c.s, g, c.d_in[0], c.d_in[1], c.d_in[2],
                     c.d_in[3], c.hprev, c.uhr, c.vhr);
  M6_HIP(hipGetLastError());
  c.tm.ms_setup += c.t_k->stop();
  return 0;
}

// the arguments of the general kernels in direction d, but for the range and the flags of the pass
void gen_args(const AdvCall &c, int d, GenArgs &a) {
  const m6::GridDev &g = c.g; const mom6hip_obc_t *obc = c.obc;
  a.g = g; a.T.ntr = c.ntr;
  for (int m = 0; m < c.ntr; m++) { a.T.t[m] = c.d_tr[m]; a.T.cu[m] = c.conc_underflow ? c.conc_underflow[m] : 0.0; }
  a.hprev = c.hprev; a.xr = d ? c.vhr : c.uhr; a.hh = c.gen_scratch; a.flux = c.gen_scratch + c.fmax_el; a.fstride = (long)c.fmax_el;
  a.domore_k = c.domore_k; a.neglect = d ? g.vh_neglect : g.uh_neglect;
  a.nseg = (int)c.gsegs[d].size(); a.segs = c.d_gsegs[d]; a.regs = c.d_gregs;
  a.obc_any = obc ? (d ? (obc->specified_v_BCs_exist_globally || obc->open_v_BCs_exist_globally)
                       : (obc->specified_u_BCs_exist_globally || obc->open_u_BCs_exist_globally)) : 0;
  a.obc_open = obc ? (d ? obc->open_v_BCs_exist_globally : obc->open_u_BCs_exist_globally) : 0;
}

// the arguments of the marching kernels for tracer group grp, but for the range and the v flags of the pass; returns the group's tracers
int group_args(const AdvCall &c, int grp, int ngroups, AdvArgs &a) {
  a.g = c.g; a.hprev = c.hprev; a.uhr = c.uhr; a.vhr = c.vhr;
  a.domore_u = c.domore_u; a.domore_k = c.domore_k;
  const int m0 = grp * MAXG;
  const int n = (c.ntr - m0 < MAXG) ? c.ntr - m0 : MAXG;
  a.any_cu = 0;
  for (int m = 0; m < MAXG; m++) {
    a.tr[m] = (m < n) ? c.d_tr[m0 + m] : nullptr;
    a.cu[m] = (m < n && c.conc_underflow) ? c.conc_underflow[m0 + m] : 0.0;
    if (a.cu[m] > 0.0) a.any_cu = 1;
  }
  a.write_mass = (grp == ngroups - 1);   // earlier groups must see the pre-pass hprev/uhr/vhr/flags
  return n;
}

// advect_x (dir 0, :329) or advect_y (dir 1, :705) over the range given: the general kernels once, or the marching kernel once a group
// of MAXG tracers.  advect_y reads domore_v and writes domore_v2 (cleared over its rows by adv_vflags_prep_kernel), and the two swap.
int adv_pass(AdvCall &c, int dir, int is, int ie, int js, int je) {
  const m6::GridDev &g = c.g; hipStream_t s = c.s; const int nz = c.nz, scheme = c.cs->scheme;
  c.t_k->start();
  if (dir) hipLaunchKernelGGL(adv_vflags_prep_kernel, dim3(64), dim3(256), 0, s, g, (const int *)c.domore_v, c.domore_v2,
                              (const int *)c.domore_k, js, je);
  int32_t &n_pass = dir ? c.tm.n_y : c.tm.n_x;
  if (c.generic) {
    GenArgs a; gen_args(c, dir, a);
    a.is = is; a.ie = ie; a.js = js; a.je = je;
    a.dom_in = dir ? c.domore_v : c.domore_u; a.dom_new = dir ? c.domore_v2 : c.gen_flags;
    if (!dir) M6_HIP(hipMemsetAsync(c.gen_flags, 0, c.nfu * sizeof(int), s));
    // a thread a face: x has ie - is + 2 faces a row, y je - js + 2 rows of faces
    const dim3 grid = dir ? dim3((ie - is + 1 + 255) / 256, je - js + 2, nz) : dim3((ie - is + 2 + 255) / 256, je - js + 1, nz);
    with_group(1, scheme, [&](auto, auto sc) {      // (the general kernels take every tracer: only the scheme is a constant)
      constexpr int SCHEME = decltype(sc)::value;
      if (dir) hipLaunchKernelGGL((gen_flux_kernel<1, SCHEME>), grid, dim3(256), 0, s, a);
      else     hipLaunchKernelGGL((gen_flux_kernel<0, SCHEME>), grid, dim3(256), 0, s, a);
    });
    if (dir) hipLaunchKernelGGL(gen_update_kernel<1>, grid, dim3(256), 0, s, a);
    else     hipLaunchKernelGGL(gen_update_kernel<0>, grid, dim3(256), 0, s, a);
    if (!dir) hipLaunchKernelGGL(gen_xflags_kernel, dim3(64), dim3(256), 0, s, g, c.domore_u, (const int *)c.gen_flags, (const int *)c.domore_k, js, je);
    M6_HIP(hipGetLastError());
    n_pass++;
  } else {
    dim3 grid((je - js + 1 + 3) / 4, nz), block(256);      // x: a wave a row, four rows a block
    int seglen = 0;
    if (dir) {      // y: a block a strip of 64 columns, its faces js-1 .. je cut into segments of at least 8, one a wave, at most YSEG
      const int nfaces = je - js + 2;
      int nseg = nfaces / 8; if (nseg < 1) nseg = 1; if (nseg > YSEG) nseg = YSEG;
      seglen = (nfaces + nseg - 1) / nseg;
      grid = dim3((ie - is + 1 + 63) / 64, nz); block = dim3(64 * nseg);
    }
    const int ngroups = (c.ntr + MAXG - 1) / MAXG;
    if (c.diag && c.diag_scratch_bytes) M6_HIP(hipMemsetAsync(c.diag_face, 0, c.diag_scratch_bytes, s));
    for (int grp = 0; grp < ngroups; grp++) {
      AdvArgs a; const int n = group_args(c, grp, ngroups, a);
      a.is = is; a.ie = ie; a.js = js; a.je = je;
      a.domore_v_in = c.domore_v; a.domore_v_out = dir ? c.domore_v2 : c.domore_v;
      AdvDiag d;
      const bool diag = c.diag && group_diag(c, grp, dir, d);
      with_group(n, scheme, [&](auto nt, auto sc) {
        constexpr int NT = decltype(nt)::value, SCHEME = decltype(sc)::value;
        if (diag) {
          if (dir) hipLaunchKernelGGL((adv_y_kernel<NT, SCHEME, true>), grid, block, 0, s, a, seglen, d);
          else     hipLaunchKernelGGL((adv_x_kernel<NT, SCHEME, true>), grid, block, 0, s, a, d);
        } else {
          if (dir) hipLaunchKernelGGL((adv_y_kernel<NT, SCHEME>), grid, block, 0, s, a, seglen, AdvNoDiag{});
          else     hipLaunchKernelGGL((adv_x_kernel<NT, SCHEME>), grid, block, 0, s, a, AdvNoDiag{});
        }
      });
      M6_HIP(hipGetLastError());
      n_pass++;
    }
    if (c.diag && c.diag_nslots)
      if (int rc = adv_diag_apply(c, dir, is, ie, js, je)) return rc;
  }
  if (dir) std::swap(c.domore_v, c.domore_v2);
  const double ms = c.t_k->stop();
  (dir ? c.tm.ms_y : c.tm.ms_x) += ms;
  if (c.itt == 1) (dir ? c.tm.ms_y1 : c.tm.ms_x1) += ms;
  return 0;
}

// do_group_pass(CS%pass_uhr_vhr_t_hprev) :206, the range that is valid after it, and domore_u / domore_v / domore_k again :215-231
int adv_group_pass(AdvCall &c) {
  const m6::GridDev &g = c.g; const int is = c.is, ie = c.ie, js = c.js, je = c.je, nz = c.nz, stencil = c.stencil;
  c.t_k->start();
  {      // (one tile: the local wrap kernels; several: the native exchange or the host's group pass)
    std::vector<double *> flds = {c.uhr, c.vhr, c.hprev};
    std::vector<int32_t> pos = {MOM6HIP_POS_U, MOM6HIP_POS_V, MOM6HIP_POS_H}, nks = {nz, nz, nz};
    for (int m = 0; m < c.ntr; m++) { flds.push_back(c.d_tr[m]); pos.push_back(MOM6HIP_POS_H); nks.push_back(nz); }
    if (int rc = m6::group_pass(c.ctx, flds.data(), pos.data(), nks.data(), (int)flds.size())) return rc;
  }
  c.halo_updates++;
  c.tm.ms_halo += c.t_k->stop();

  const int nsten_halo = std::min({is - g.isd, g.ied - ie, js - g.jsd, g.jed - je}) / stencil;
  c.isv = is - nsten_halo * stencil; c.jsv = js - nsten_halo * stencil;
  c.iev = ie + nsten_halo * stencil; c.jev = je + nsten_halo * stencil;
  if ((nsten_halo > 1) || (c.itt == 1)) {
    const int isv = c.isv, iev = c.iev, jsv = c.jsv, jev = c.jev;
    c.t_k->start();
    ScanArgs sa;
    sa.g = g; sa.uhr = c.uhr; sa.vhr = c.vhr; sa.domore_u = c.domore_u; sa.domore_v = c.domore_v; sa.domore_k = c.domore_k;
    sa.ju0 = jsv; sa.ju1 = jev; sa.iu0 = isv + stencil - 1; sa.iu1 = iev - stencil;
    sa.jv0 = jsv + stencil - 1; sa.jv1 = jev - stencil; sa.iv0 = isv + stencil; sa.iv1 = iev - stencil;
    hipLaunchKernelGGL(adv_scan_kernel, dim3(g.njh + 1, nz), dim3(256), 0, c.s, sa);
    hipLaunchKernelGGL(adv_domore_k_kernel, dim3(nz), dim3(64), 0, c.s, g, (const int *)c.domore_u,
                       (const int *)c.domore_v, c.domore_k, jsv, jev, jsv + stencil - 1, jev - stencil);
    M6_HIP(hipGetLastError());
    c.tm.ms_setup += c.t_k->stop();
  }
  return 0;
}

// one iteration's two passes on the range a stencil narrower, and domore_k of the rows they worked on (:233-289)
int adv_sweep(AdvCall &c) {
  const int stencil = c.stencil;
  c.isv += stencil; c.iev -= stencil; c.jsv += stencil; c.jev -= stencil;
  const int isv = c.isv, iev = c.iev, jsv = c.jsv, jev = c.jev;
  int ju0 = jsv, ju1 = jev;      // the rows of advect_x
  if (c.x_first) {
    ju0 = jsv - stencil; ju1 = jev + stencil;
    if (int rc = adv_pass(c, 0, isv, iev, ju0, ju1)) return rc;
    if (int rc = adv_pass(c, 1, isv, iev, jsv, jev)) return rc;
  } else {
    if (int rc = adv_pass(c, 1, isv - stencil, iev + stencil, jsv, jev)) return rc;
    if (int rc = adv_pass(c, 0, isv, iev, jsv, jev)) return rc;
  }
  hipLaunchKernelGGL(adv_domore_k_kernel, dim3(c.nz), dim3(64), 0, c.s, c.g, (const int *)c.domore_u, (const int *)c.domore_v,
                     c.domore_k, ju0, ju1, jsv - 1, jev);
  M6_HIP(hipGetLastError());
  return 0;
}

// c.remaining = sum(domore_k); across_PEs: sum_across_PEs(domore_k) first, :305 -- the one host read-back per iteration
int adv_count_remaining(AdvCall &c, bool across_PEs) {
  mom6hip_ctx_t *ctx = c.ctx; const int nz = c.nz;
  if (across_PEs && m6::multi_tile(ctx)) {
    // domore_k becomes the global count and is what the next iteration tests (:215, :252): reduced where it lies (an all-reduce on the
    // communication stream with the native domain), the host's copy read back behind it
    if (int rc = m6::sum_across_PEs_dev(ctx, c.domore_k, nz, ctx->h_domore_k)) return rc;
  } else {
    M6_HIP(hipMemcpyAsync(ctx->h_domore_k, c.domore_k, nz * sizeof(int), hipMemcpyDeviceToHost, c.s));
    M6_HIP(hipStreamSynchronize(c.s));
  }
  c.remaining = 0;
  for (int k = 0; k < nz; k++) c.remaining += ctx->h_domore_k[k];
  return 0;
}

// the tracers, uhr, vhr and vol_prev back to the caller; the statistics
int adv_outputs(AdvCall &c, mom6hip_advect_stats_t *stats) {
  hipStream_t s = c.s;
  const hipMemcpyKind kind = (c.memspace == MOM6HIP_MEM_HOST) ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  if (c.memspace == MOM6HIP_MEM_HOST)
    for (int m = 0; m < c.ntr; m++) M6_HIP(hipMemcpyAsync(c.tr[m], c.d_tr[m], c.bH, kind, s));
  if (c.uhr_out) M6_HIP(hipMemcpyAsync(c.uhr_out, c.uhr, c.bU, kind, s));
  if (c.vhr_out) M6_HIP(hipMemcpyAsync(c.vhr_out, c.vhr, c.bV, kind, s));
  if (c.vol_prev && c.update_vol_prev) M6_HIP(hipMemcpyAsync(c.vol_prev, c.hprev, c.bH, kind, s));
  if (c.diag && c.memspace == MOM6HIP_MEM_HOST) {
    const size_t bytes[5] = {c.bU, c.bV, c.bU / c.nz, c.bV / c.nz, c.bH};
    for (int m = 0; m < c.ntr; m++) {
      double *const dst[5] = {c.diag[m].ad_x, c.diag[m].ad_y, c.diag[m].ad2d_x, c.diag[m].ad2d_y, c.diag[m].advection_xy};
      for (int q = 0; q < 5; q++) if (dst[q]) M6_HIP(hipMemcpyAsync(dst[q], c.d_diag[m][q], bytes[q], kind, s));
    }
  }
  if (stats || c.memspace == MOM6HIP_MEM_HOST)      // (the copies are complete behind it)
    if (int rc = adv_count_remaining(c, false)) return rc;
  if (stats) { stats->iterations = c.itt; stats->halo_updates = c.halo_updates; stats->domore_remaining = c.remaining; }
  return 0;
}

}  // namespace

extern "C" int mom6hip_advect_get_timing(mom6hip_ctx_t *ctx, mom6hip_advect_timing_t *t) {
  M6_REQUIRE(ctx && t, "mom6hip_advect_get_timing: null argument");
  *t = ctx->adv_timing;
  return 0;
}

extern "C" int mom6hip_advect_tracer(mom6hip_ctx_t *ctx, const double *h_end, const double *uhtr, const double *vhtr, double dt,
                                     const mom6hip_tracer_advect_cs_t *cs, double *const *tr, const double *conc_underflow, int32_t ntr,
                                     int32_t x_first_in, double *vol_prev, int32_t max_iter_in, int32_t update_vol_prev, double *uhr_out,
                                     double *vhr_out, int32_t memspace, mom6hip_advect_stats_t *stats) {
  return mom6hip_advect_tracer_obc(ctx, h_end, uhtr, vhtr, dt, cs, tr, conc_underflow, ntr, x_first_in, vol_prev, max_iter_in, update_vol_prev,
                                   uhr_out, vhr_out, nullptr, memspace, stats);
}

// advect_tracer with OBC associated: of the OBC, advect_x / advect_y read the tracer registries of the segments (segment%tr_Reg); without
// any the marching kernels run as for a closed domain, with one the general kernels (gen_flux_kernel, gen_update_kernel)
extern "C" int mom6hip_advect_tracer_obc(mom6hip_ctx_t *ctx, const double *h_end, const double *uhtr, const double *vhtr, double dt,
                                         const mom6hip_tracer_advect_cs_t *cs, double *const *tr, const double *conc_underflow, int32_t ntr,
                                         int32_t x_first_in, double *vol_prev, int32_t max_iter_in, int32_t update_vol_prev, double *uhr_out,
                                         double *vhr_out, const mom6hip_obc_t *obc, int32_t memspace, mom6hip_advect_stats_t *stats) {
  return mom6hip_advect_tracer_diag(ctx, h_end, uhtr, vhtr, dt, cs, tr, conc_underflow, ntr, x_first_in, vol_prev, max_iter_in, update_vol_prev,
                                    uhr_out, vhr_out, obc, memspace, stats, nullptr);
}

// the same with the flux diagnostics of the tracers (diag: null, or a record a tracer; adv_diag_setup, group_diag, adv_diag_apply)
extern "C" int mom6hip_advect_tracer_diag(mom6hip_ctx_t *ctx, const double *h_end, const double *uhtr, const double *vhtr, double dt,
                                          const mom6hip_tracer_advect_cs_t *cs, double *const *tr, const double *conc_underflow, int32_t ntr,
                                          int32_t x_first_in, double *vol_prev, int32_t max_iter_in, int32_t update_vol_prev, double *uhr_out,
                                          double *vhr_out, const mom6hip_obc_t *obc, int32_t memspace, mom6hip_advect_stats_t *stats,
                                          const mom6hip_tracer_flux_diag_t *diag) {
  M6_REQUIRE(ctx != nullptr, "advect_tracer: null context (tracer_advect_init must be called before advect_tracer)");
  if (stats) memset(stats, 0, sizeof(*stats));
  M6_REQUIRE(ntr >= 0, "advect_tracer: ntr < 0");
  if (ntr == 0) return 0;   // :124
  AdvCall c{};      // (every scalar and pointer zero until its phase sets it)
  c.ctx = ctx; c.cs = cs; c.obc = obc; c.s = ctx->stream; c.g = ctx->g;
  c.h_end = h_end; c.uhtr = uhtr; c.vhtr = vhtr; c.conc_underflow = conc_underflow; c.tr = tr; c.vol_prev = vol_prev;
  c.uhr_out = uhr_out; c.vhr_out = vhr_out; c.ntr = ntr; c.memspace = memspace; c.update_vol_prev = update_vol_prev;
  c.diag = diag; c.Idt = 1.0 / dt;      // :133
  int rc = 0;
  if ((rc = adv_check(c, dt, x_first_in, max_iter_in))) return rc;

  Timer t_all(ctx->timing, c.s), t_k(ctx->timing, c.s);
  c.t_k = &t_k;
  t_all.start();
  if ((rc = adv_stage_in(c))) return rc;
  if ((rc = adv_work_space(c))) return rc;
  if ((rc = adv_registries(c))) return rc;
  if ((rc = adv_diag_setup(c))) return rc;                   // :190-198
  if ((rc = adv_setup(c))) return rc;                        // :152-178

  c.isv = c.is; c.iev = c.ie; c.jsv = c.js; c.jev = c.je;
  c.remaining = c.nz;
  for (c.itt = 1; c.itt <= c.max_iter; c.itt++) {            // :203
    const bool narrow = c.isv > c.is - c.stencil;            // the halo that is valid is used up
    if (narrow && (rc = adv_group_pass(c))) return rc;       // :206-231
    if ((rc = adv_sweep(c))) return rc;                      // :233-289
    if (c.itt >= c.max_iter) break;
    if (c.isv > c.is - c.stencil) {                          // :303-307
      if ((rc = adv_count_remaining(c, true))) return rc;
      if (c.remaining == 0) break;
    }
  }
  if (c.itt > c.max_iter) c.itt = c.max_iter;

  if ((rc = adv_outputs(c, stats))) return rc;
  if (ctx->timing) { c.tm.ms_total = t_all.stop(); ctx->adv_timing = c.tm; }
  return 0;
}
