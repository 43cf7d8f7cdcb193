// remap_pieces.hpp -- the per-cell pieces of remapping_core_h's vertical reconstructions (src/ALE/PLM_functions.F90, PPM_functions.F90,
// regrid_edge_values.F90, regrid_solvers.F90, MOM_remapping.F90), one text for the three files that use them: ale_remap.hip (the
// streaming kernel's register window and the wave path's LDS column), hor_bnd_diffusion.hip (a lane's private column) and
// pressure_force.hip (the PLM edge values of T and S).  Scalar functions, values in and values out with the assignment left at the
// call, and the few serial routines over plain pointers that one lane runs.  The line numbers are the reference's.
//
// Two flavours of minimum and maximum.  The pieces take them by the names rmin / rmax, and a file says which it means before it
// includes this header:
//   #define REMAP_PIECES_SELECT 1   m6::min2 / max2, compare-and-select (a < b ? a : b): what the oracle writes, and what
//                                   hor_bnd_diffusion.hip and pressure_force.hip have always used;
//   #define REMAP_PIECES_SELECT 0   fmin / fmax, one v_min_f64 / v_max_f64 each: what the ALE kernels have always used; they are on
//                                   the benchmark's path.
// The two differ only for a (-0.0, +0.0) pair and for NaN.  Horizontal boundary diffusion is tested with a tracer of -0.0
// (tests/test_hor_bnd_diffusion.py, test_tracer_hordiff_hbd_negative_zero_tracer_matches_checker) and keeps select; moving the ALE
// kernels to select would change their instructions, and possibly their bits, which is a question of behaviour and not of layout.
// Every .hip file is a translation unit of its own and everything here lives in the anonymous namespace, so the flavours never meet.
//
// implicit_h4_row, h4cw_slope, h4cw_edge, ppm_monotonicity_cell and average_value_ppoly are called by hor_bnd_diffusion.hip alone:
// ale_remap.hip's wave path keeps the same arithmetic written out in w_edges_implicit_h4, w_edges_h4cw and w_average_value_ppoly,
// because a call of any one of the five there changes ale_remap_wave_kernel's instructions (profiles/remap_pieces.txt, section 3).
// A change to one of the five is made in both places.
#pragma once
#include <cfloat>
#include <cmath>

#include "common.hpp"

#if !defined(REMAP_PIECES_SELECT)
#error "define REMAP_PIECES_SELECT as 1 (m6::min2 / max2) or 0 (fmin / fmax) before including remap_pieces.hpp"
#endif

namespace {

#if REMAP_PIECES_SELECT
__device__ __forceinline__ double rmin(double a, double b) { return m6::min2(a, b); }
__device__ __forceinline__ double rmax(double a, double b) { return m6::max2(a, b); }
#else
__device__ __forceinline__ double rmin(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ double rmax(double a, double b) { return fmax(a, b); }
#endif

constexpr int INT_PCM = 0, INT_PLM = 1, INT_PPM = 3, INT_PQM = 5;   // MOM_remapping.F90:61-64

// The scheme build_reconstructions_1d uses on a column of n cells (MOM_remapping.F90:283-296; MOM6HIP_REMAP_* are :50-59's numbers)
__host__ __device__ inline int remap_local_scheme(int scheme, int n) {
  if (n <= 1) return MOM6HIP_REMAP_PCM;
  if (n <= 3) return (scheme < MOM6HIP_REMAP_PLM) ? scheme : MOM6HIP_REMAP_PLM;
  if (n <= 4 && scheme != MOM6HIP_REMAP_PPM_CW) return (scheme < MOM6HIP_REMAP_PPM_H4) ? scheme : MOM6HIP_REMAP_PPM_H4;      // :293
  return scheme;
}

__device__ __forceinline__ double max3(double a, double b, double c) { return rmax(rmax(a, b), c); }
__device__ __forceinline__ double min3(double a, double b, double c) { return rmin(rmin(a, b), c); }
__device__ __forceinline__ double fsign(double a, double b) { return copysign(fabs(a), b); }

// ---- PLM_functions.F90 ----------------------------------------------------------------------------
// PLM_slope_wa :22-65
__device__ double plm_slope_wa(double h_l, double h_c, double h_r, double h_neglect, double u_l, double u_c, double u_r) {
  const double sigma_r = u_r - u_c;
  const double sigma_l = u_c - u_l;
  const double sigma_c = 2.0 * (u_r - u_l) * (h_c / (h_l + 2.0 * h_c + h_r + h_neglect));
  const double u_min = min3(u_l, u_c, u_r);
  const double u_max = max3(u_l, u_c, u_r);
  double slope = 0.0;
  if ((sigma_l * sigma_r) > 0.0) slope = fsign(rmin(fabs(sigma_c), 2. * rmin(u_c - u_min, u_max - u_c)), sigma_c);
  if (u_c - 0.5 * fabs(slope) < u_min || u_c + 0.5 * fabs(slope) > u_max) slope = slope * (1. - DBL_EPSILON);
  if (fabs(slope) < 1.E-140) slope = 0.;
  return slope;
}

// PLM_monotonized_slope :124-159
__device__ double plm_monotonized_slope(double u_l, double u_c, double u_r, double s_l, double s_c, double s_r) {
  const double almost_two = 2. * (1. - DBL_EPSILON);
  const double e_r = u_l + 0.5 * s_l;
  const double e_l = u_r - 0.5 * s_r;
  double slp = fabs(s_c);
  double edge = u_c - 0.5 * s_c;
  if ((edge - e_r) * (u_c - edge) < 0.) {
    edge = 0.5 * (edge + e_r);
    slp = rmin(slp, fabs(edge - u_c) * almost_two);
  }
  edge = u_c + 0.5 * s_c;
  if ((edge - u_c) * (e_l - edge) < 0.) {
    edge = 0.5 * (edge + e_l);
    slp = rmin(slp, fabs(edge - u_c) * almost_two);
  }
  return fsign(slp, s_c);
}

// PLM_extrapolate_slope :164-183
__device__ double plm_extrapolate_slope(double h_l, double h_c, double h_neglect, double u_l, double u_c) {
  const double hl = h_l + h_neglect;
  const double hc = h_c + h_neglect;
  const double left_edge = (u_l * hc + u_c * hl) / (hl + hc);
  return 2.0 * (u_c - left_edge);
}

// PLM_boundary_extrapolation :272-307 on a column's edge values EL, ER and slope column C1 (ppoly_coef(:,2); coef(:,1) is EL), by one lane
__device__ void plm_boundary_extrapolation(const double *h, const double *u, double *EL, double *ER, double *C1, int n, double h_neglect) {
  double slope = -plm_extrapolate_slope(h[1], h[0], h_neglect, u[1], u[0]);
  EL[0] = u[0] - 0.5 * slope; ER[0] = u[0] + 0.5 * slope;
  C1[0] = ER[0] - EL[0];
  slope = plm_extrapolate_slope(h[n - 2], h[n - 1], h_neglect, u[n - 2], u[n - 1]);
  EL[n - 1] = u[n - 1] - 0.5 * slope; ER[n - 1] = u[n - 1] + 0.5 * slope;
  C1[n - 1] = ER[n - 1] - EL[n - 1];
}

// ---- regrid_edge_values.F90 -----------------------------------------------------------------------
// end_value_h4 :658-771
__device__ void end_value_h4(const double dz[4], const double u[4], double Csys[4]) {
  const double min_frac = 1.0e-6;
  double h1 = dz[0], h2 = dz[1], h3 = dz[2], h4 = dz[3];
  if ((h2 + h3) < min_frac * h1) h3 = min_frac * h1 - h2;
  if ((h3 + h4) < min_frac * h1) h4 = min_frac * h1 - h3;
  const double h12 = h1 + h2, h23 = h2 + h3, h34 = h3 + h4;
  const double h123 = h12 + h3, h234 = h2 + h34, h1234 = h12 + h34;
  const double I_denB3 = 1.0 / (h123 * h12 * h23);
  const double I_h12 = (h123 * h23) * I_denB3;
  const double I_h23 = (h12 * h123) * I_denB3;
  const double I_h123 = (h12 * h23) * I_denB3;
  const double I_denom = 1.0 / (h1234 * (h234 * h34));
  const double I_h234 = (h1234 * h34) * I_denom;
  const double I_h1234 = (h234 * h34) * I_denom;

  const double W11 = -h1 * (I_h1234 + I_h123 + I_h12);
  const double W21 = h1 * h12 * (I_h234 * I_h1234 + I_h23 * (I_h234 + I_h123));
  const double W31 = -h1 * h12 * h123 * I_denom;
  const double W12 = 2.0 * (I_h12 * (1.0 + (h1 + h12) * (I_h1234 + I_h123)) + h1 * I_h1234 * I_h123);
  const double W22 = -2.0 * ((h1 * h12 * I_h1234) * (I_h23 * (I_h234 + I_h123)) +
                             (h1 + h12) * (I_h1234 * I_h234 + I_h23 * (I_h234 + I_h123)));
  const double W32 = 2.0 * ((h1 + h12) * h123 + h1 * h12) * I_denom;
  const double W13 = -3.0 * I_h12 * I_h123 * (1.0 + I_h1234 * ((h1 + h12) + h123));
  const double W23 = 3.0 * I_h23 * (I_h123 + I_h1234 * ((h1 + h12) + h123) * (I_h123 + I_h234));
  const double W33 = -3.0 * ((h1 + h12) + h123) * I_denom;
  const double W14 = 4.0 * I_h1234 * I_h123 * I_h12;
  const double W24 = -4.0 * I_h1234 * (I_h23 * (I_h123 + I_h234));
  const double W34 = 4.0 * I_denom;

  Csys[0] = ((u[0] + W11 * (u[1] - u[0])) + W21 * (u[2] - u[1])) + W31 * (u[3] - u[2]);
  Csys[1] = (W12 * (u[1] - u[0]) + W22 * (u[2] - u[1])) + W32 * (u[3] - u[2]);
  Csys[2] = (W13 * (u[1] - u[0]) + W23 * (u[2] - u[1])) + W33 * (u[3] - u[2]);
  Csys[3] = (W14 * (u[1] - u[0]) + W24 * (u[2] - u[1])) + W34 * (u[3] - u[2]);
}

// The cubic of end_value_h4 through the first (last = false) or the last four cells of a column, counted from the end, their widths
// floored at hNeglect (:329-362, :619-640); returns the floored width of the end cell
__device__ double end_polynomial_h4(const double *h, const double *u, bool last, int n, double hNeglect, double Cs[4]) {
  double dz[4], ut[4];
  for (int i = 0; i < 4; i++) { const int q = last ? n - 1 - i : i; dz[i] = rmax(hNeglect, h[q]); ut[i] = u[q]; }
  end_value_h4(dz, ut, Cs);
  return dz[0];
}

struct EdgeW { double A1, A2, B, Cc, Hs; };
// the thickness-only factors of edge_values_explicit_h4 (regrid_edge_values.F90:262-300) at the interface above cell i
__device__ __forceinline__ EdgeW edge_weights_h4(double h0, double h1, double h2, double h3, double hNeglect) {
  const double hMinFrac = 1.e-5;
  if (h0 + h1 == 0.0 || h1 + h2 == 0.0 || h2 + h3 == 0.0) {
    const double h_min = hMinFrac * rmax(hNeglect, (h0 + h1) + (h2 + h3));
    h0 = rmax(h_min, h0); h1 = rmax(h_min, h1); h2 = rmax(h_min, h2); h3 = rmax(h_min, h3);
  }
  const double I_h12 = 1.0 / (h1 + h2);
  const double I_den_et2 = 1.0 / (((h0 + h1) + h2) * (h0 + h1)); const double I_h012 = (h0 + h1) * I_den_et2;
  const double I_den_et3 = 1.0 / ((h1 + (h2 + h3)) * (h2 + h3)); const double I_h123 = (h2 + h3) * I_den_et3;
  EdgeW w;
  w.A1 = (1.0 + (h1 * I_h012 + (h0 + h1) * I_h123)) * I_h12 * (h2 * (h2 + h3));
  w.A2 = (1.0 + (h2 * I_h123 + (h2 + h3) * I_h012)) * I_h12 * (h1 * (h0 + h1));
  w.B = (h1 * (h2 * (h2 + h3)) * I_den_et2);
  w.Cc = (h2 * (h1 * (h0 + h1)) * I_den_et3);
  w.Hs = (h0 + h1) + (h2 + h3);
  return w;
}
__device__ __forceinline__ double edge_value_h4(const EdgeW &w, double um2, double um1, double u0, double up1) {
  const double et1 = w.A1 * um1 + w.A2 * u0;
  const double et2 = w.B * (um1 - um2);
  const double et3 = w.Cc * (u0 - up1);
  return (et1 + (et2 + et3)) / w.Hs;
}
// the row of edge_values_implicit_h4's tridiagonal system (:560-590, answer_date >= 20190101) for the interface between two cells of
// widths h0, h1 and means u0, u1
struct TriRow { double l, c, u, b; };
__device__ __forceinline__ TriRow implicit_h4_row(double h0, double h1, double u0, double u1, double hNeglect) {
  h0 = rmax(h0, hNeglect);
  h1 = rmax(h1, hNeglect);
  if (fabs(h0) < 1.0e-12 * fabs(h1)) h0 = 1.0e-12 * h1;
  if (fabs(h1) < 1.0e-12 * fabs(h0)) h1 = 1.0e-12 * h0;
  const double I_h2 = 1.0 / ((h0 + h1) * (h0 + h1));
  const double alpha = (h1 * h1) * I_h2;
  const double beta = (h0 * h0) * I_h2;
  const double abmix = (h0 * h1) * I_h2;
  const double a = 2.0 * alpha * (alpha + 2.0 * beta + 3.0 * abmix);
  const double b = 2.0 * beta * (beta + 2.0 * alpha + 3.0 * abmix);
  TriRow r;
  r.c = 2.0 * abmix; r.l = alpha; r.u = beta;
  r.b = a * u0 + b * u1;
  return r;
}
// edge_values_explicit_h4cw :381-463.  The limited slope au(k) of Colella & Woodward eq. 1.8 for a cell of floored width dp_c and mean u_c
// between its two neighbours (h2_h123(k), h112(K), I_h12(K+1), h122(K+1), I_h12(K) of the reference with K = k+1)
__device__ __forceinline__ double h4cw_slope(double dp_l, double dp_c, double dp_r, double u_l, double u_c, double u_r) {
  const double slk = u_c - u_l;
  const double srk = u_r - u_c;
  if (!(slk * srk > 0.)) return 0.;
  const double h2_h123 = dp_c / (dp_c + (dp_l + dp_r));
  const double h112 = 2. * dp_l + dp_c, h122p = dp_c + 2. * dp_r;
  const double I_h12 = 1.0 / (dp_l + dp_c), I_h12p = 1.0 / (dp_c + dp_r);
  const double sck = h2_h123 * (h112 * srk * I_h12p + h122p * slk * I_h12);
  return fsign(min3(fabs(2.0 * slk), fabs(sck), fabs(2.0 * srk)), sck);
}
// ... and al(k), the edge between cells k-1 and k, from the floored widths of cells k-2 .. k+1, the means and the limited slopes of k-1, k
__device__ __forceinline__ double h4cw_edge(double dp_m2, double dp_m1, double dp_0, double dp_p1, double u_m1, double u_0, double au_m1,
                                            double au_0) {
  const double I_h12 = 1.0 / (dp_m1 + dp_0);
  const double I_h0123 = 1.0 / ((dp_m2 + dp_m1) + (dp_0 + dp_p1));
  const double h01_h112 = (dp_m2 + dp_m1) / (2.0 * dp_m1 + dp_0);
  const double h23_h122 = (dp_0 + dp_p1) / (dp_m1 + 2.0 * dp_0);
  return (dp_0 * u_m1 + dp_m1 * u_0) * I_h12 +
         I_h0123 * (2. * dp_0 * dp_m1 * I_h12 * (u_0 - u_m1) * (h01_h112 - h23_h122) + (dp_0 * au_m1 * h23_h122 - dp_m1 * au_0 * h01_h112));
}
// the slope of bound_edge_values (regrid_edge_values.F90:71-82) with hr = h(k) / ((h(km1) + h(kp1)) + 2 h(k)) or a negative hr for "no slope"
__device__ __forceinline__ double bound_slope(double ukm1, double uk, double ukp1, double hr) {
  double slope_x_h = 0.0;
  if (hr >= 0.0) {
    const double sigma_l = (uk - ukm1);
    const double sigma_c = (ukp1 - ukm1) * hr;
    const double sigma_r = (ukp1 - uk);
    if ((sigma_l * sigma_r) > 0.0) slope_x_h = fsign(min3(fabs(sigma_l), fabs(sigma_c), fabs(sigma_r)), sigma_c);
  }
  return slope_x_h;
}
__device__ __forceinline__ double bound_left(double EL, double ukm1, double uk, double slope) {
  if ((ukm1 - EL) * (EL - uk) < 0.0) EL = uk - fsign(rmin(fabs(slope), fabs(EL - uk)), slope);
  return rmax(rmin(EL, rmax(ukm1, uk)), rmin(ukm1, uk));
}
__device__ __forceinline__ double bound_right(double ER, double ukp1, double uk, double slope) {
  if ((ukp1 - ER) * (ER - uk) < 0.0) ER = uk + fsign(rmin(fabs(slope), fabs(ER - uk)), slope);
  return rmax(rmin(ER, rmax(ukp1, uk)), rmin(ukp1, uk));
}
// check_discontinuous_edge_values :141-159 at the interface between cells k and k+1 (er the right edge of k, el_next the left edge of
// k+1): the test, and the value both edges take when it holds
__device__ __forceinline__ bool edges_discontinuous(double u_k, double u_kp1, double er, double el_next) {
  return (el_next - er) * (u_kp1 - u_k) < 0.0;
}
__device__ __forceinline__ double bounded_edge_average(double u_k, double u_kp1, double er, double el_next) {
  const double u0_avg = 0.5 * (er + el_next);
  return rmax(rmin(u0_avg, rmax(u_k, u_kp1)), rmin(u_k, u_kp1));
}

// ---- regrid_solvers.F90 ---------------------------------------------------------------------------
// solve_diag_dominant_tridiag :246-280 as a serial walk by one lane; the solution overwrites the right-hand side, c1 is work space
__device__ void solve_diag_dominant_tridiag(const double *tri_l, const double *tri_c, const double *tri_u, double *tri_b, double *c1, int N) {
  double I_pivot = 1.0 / (tri_c[0] + tri_u[0]);
  double d1 = tri_c[0] * I_pivot;
  c1[0] = tri_u[0] * I_pivot;
  tri_b[0] = tri_b[0] * I_pivot;
  for (int k = 1; k < N - 1; k++) {
    const double denom_t1 = tri_c[k] + d1 * tri_l[k];
    I_pivot = 1.0 / (denom_t1 + tri_u[k]);
    d1 = denom_t1 * I_pivot;
    c1[k] = tri_u[k] * I_pivot;
    tri_b[k] = (tri_b[k] - tri_l[k] * tri_b[k - 1]) * I_pivot;
  }
  I_pivot = 1.0 / (tri_c[N - 1] + d1 * tri_l[N - 1]);
  tri_b[N - 1] = (tri_b[N - 1] - tri_l[N - 1] * tri_b[N - 2]) * I_pivot;
  for (int k = N - 2; k >= 0; k--) tri_b[k] = tri_b[k] - c1[k] * tri_b[k + 1];
}

// ---- PPM_functions.F90, MOM_remapping.F90 -----------------------------------------------------------
// PPM_limiter_standard for an interior cell (PPM_functions.F90:84-121)
__device__ __forceinline__ void ppm_limit_cell(double u_l, double u_c, double u_r, double &edge_l, double &edge_r) {
  if ((u_r - u_c) * (u_c - u_l) <= 0.0) {
    edge_l = u_c; edge_r = u_c;
  } else {
    const double expr1 = 3.0 * (edge_r - edge_l) * ((u_c - edge_l) + (u_c - edge_r));
    const double expr2 = (edge_r - edge_l) * (edge_r - edge_l);
    if (expr1 > expr2) {
      edge_l = u_c + 2.0 * (u_c - edge_r);
      edge_l = rmax(rmin(edge_l, rmax(u_l, u_c)), rmin(u_l, u_c));
    } else if (expr1 < -expr2) {
      edge_r = u_c + 2.0 * (u_c - edge_l);
      edge_r = rmax(rmin(edge_r, rmax(u_r, u_c)), rmin(u_r, u_c));
    }
  }
  if (fabs(edge_r - edge_l) < rmax(1.e-60, DBL_EPSILON * fabs(u_c))) { edge_l = u_c; edge_r = u_c; }
}
// PPM_monotonicity for an interior cell (PPM_functions.F90:132-158)
__device__ __forceinline__ void ppm_monotonicity_cell(double u_l, double u_c, double u_r, double &edge_l, double &edge_r) {
  if ((u_r - u_c) * (u_c - u_l) <= 0.) {
    edge_l = u_c; edge_r = u_c;
  } else {
    const double da = edge_r - edge_l;
    const double a6 = 6.0 * u_c - 3.0 * (edge_l + edge_r);
    if (da * a6 > da * da) edge_l = 3.0 * u_c - 2.0 * edge_r;
    else if (da * a6 < -da * da) edge_r = 3.0 * u_c - 2.0 * edge_l;
  }
}
// PPM_boundary_extrapolation (PPM_functions.F90:162-316) on a column's edge values and slope column, by one lane; coef(:,3) of the
// last cell but one is formed from its edges by the expression that defined it
__device__ void ppm_boundary_extrapolation(const double *h, const double *u, double *EL, double *ER, double *C1, int n, double h_neglect) {
  int i0 = 0, i1 = 1;
  double h0 = h[i0], h1 = h[i1], u0 = u[i0], u1 = u[i1];
  double b = C1[i1];
  double u1_r = b * ((h0 + h_neglect) / (h1 + h_neglect));
  double slope = 2.0 * (u1 - u0);
  if (fabs(u1_r) > fabs(slope)) u1_r = slope;
  double u0_r = EL[i1];
  double u0_l = 3.0 * u0 + 0.5 * u1_r - 2.0 * u0_r;
  double exp1 = (u0_r - u0_l) * (u0 - 0.5 * (u0_l + u0_r));
  double exp2 = (u0_r - u0_l) * (u0_r - u0_l) / 6.0;
  if (exp1 > exp2) u0_l = 3.0 * u0 - 2.0 * u0_r;
  if (exp1 < -exp2) u0_r = 3.0 * u0 - 2.0 * u0_l;
  EL[i0] = u0_l; ER[i0] = u0_r;
  C1[i0] = 6.0 * u0 - 4.0 * u0_l - 2.0 * u0_r;
  i0 = n - 2; i1 = n - 1;
  h0 = h[i0]; h1 = h[i1]; u0 = u[i0]; u1 = u[i1];
  b = C1[i0];
  const double cc = 3.0 * ((ER[i0] - u[i0]) + (EL[i0] - u[i0]));      // ppoly_coef(i0,3)
  double u1_l = (b + 2 * cc);
  u1_l = u1_l * ((h1 + h_neglect) / (h0 + h_neglect));
  slope = 2.0 * (u1 - u0);
  if (fabs(u1_l) > fabs(slope)) u1_l = slope;
  u0_l = ER[i0];
  u0_r = 3.0 * u1 - 0.5 * u1_l - 2.0 * u0_l;
  exp1 = (u0_r - u0_l) * (u1 - 0.5 * (u0_l + u0_r));
  exp2 = (u0_r - u0_l) * (u0_r - u0_l) / 6.0;
  if (exp1 > exp2) u0_l = 3.0 * u1 - 2.0 * u0_r;
  if (exp1 < -exp2) u0_r = 3.0 * u1 - 2.0 * u0_l;
  EL[i1] = u0_l; ER[i1] = u0_r;
  C1[i1] = 6.0 * u1 - 4.0 * u0_l - 2.0 * u0_r;
}
// average_value_ppoly for INT_PPM (MOM_remapping.F90:998-1099)
__device__ __forceinline__ double average_ppm(double a_L, double a_R, double u_c, double xa, double xb) {
  if (xb > xa) {
    const double mx = 0.5 * (xa + xb);
    const double a_c = 0.5 * ((u_c - a_L) + (u_c - a_R));
    if (mx < 0.5) {
      const double xa2b2ab = (xa * xa + xb * xb) + xa * xb;
      return a_L + ((a_R - a_L) * mx + a_c * (3. * (xb + xa) - 2. * xa2b2ab));
    } else {
      const double Ya = 1. - xa, Yb = 1. - xb;
      const double my = 0.5 * (Ya + Yb);
      const double Ya2b2ab = (Ya * Ya + Yb * Yb) + Ya * Yb;
      return a_R + ((a_L - a_R) * my + a_c * (3. * (Yb + Ya) - 2. * Ya2b2ab));
    }
  }
  const double Ya = 1. - xa;
  const double a_c = 3. * ((u_c - a_L) + (u_c - a_R));
  if (xa < 0.5) return a_L + xa * ((a_R - a_L) + a_c * Ya);
  return a_R + Ya * ((a_L - a_R) + a_c * xa);
}
// average_value_ppoly :998-1099 for INT_PCM, INT_PLM and INT_PPM, from the cell's mean, its edge values and its slope c1 = ppoly_coef(:,2)
__device__ __forceinline__ double average_value_ppoly(int method, double u_c, double a_L, double a_R, double c1, double xa, double xb) {
  if (method == INT_PCM) return (xb > xa) ? u_c : a_L;
  if (method == INT_PLM) {
    if (xb > xa) return (a_L + c1 * 0.5 * (xb + xa));
    if (xa < 0.5) return a_L + xa * (a_R - a_L);
    return a_R + (1. - xa) * (a_L - a_R);
  }
  return average_ppm(a_L, a_R, u_c, xa, xb);
}

}  // namespace
