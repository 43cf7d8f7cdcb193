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
// One lane per face walks the serial depth loops of its column pair from private arrays (sized by the template's layer bound NKM).
// The vertical reconstructions are those of remapping_core_h (src/ALE/MOM_remapping.F90:160) for PCM, PLM, PPM_H4, PPM_IH4 and
// PPM_CW, with and without boundary extrapolation, force_bounds_in_subcell = .false.; they are restated here on their own and
// leave the ALE kernels (ale_remap.hip) untouched.
// Algorithmic traffic per tracer and iteration: the flux kernels read h and the tracer of both columns of every wet face down to the
// HBD grid's depth and write nflx_max planes of fluxes per direction; the update reads h and the fluxes and reads and writes every
// layer of the tracer (>= 24 B per cell).
#include <cfloat>
#include <cmath>

#include "common.hpp"

namespace {

using m6::max2;
using m6::min2;

__device__ __forceinline__ double max3(double a, double b, double c) { return max2(max2(a, b), c); }
__device__ __forceinline__ double min3(double a, double b, double c) { return min2(min2(a, b), c); }
__device__ __forceinline__ double fsign(double a, double b) { return copysign(fabs(a), b); }

enum { INT_PCM = 0, INT_PLM = 1, INT_PPM = 3 };

// ---- reconstructions (E[s*n + k], coef[d*n + k]; k 0-based) ---------------------------------------------------------------
#define E_(k, s) E[(s) * n + (k)]
#define C_(k, d) coef[(d) * n + (k)]

// PLM_slope_wa, src/ALE/PLM_functions.F90:22-65
__device__ double plm_slope_wa(double h_l, double h_c, double h_r, double h_neglect, double u_l, double u_c, double u_r) {
  const double sigma_r = u_r - u_c;
  const double sigma_l = u_c - u_l;
  const double sigma_c = 2.0 * (u_r - u_l) * (h_c / (h_l + 2.0 * h_c + h_r + h_neglect));
  const double u_min = min3(u_l, u_c, u_r);
  const double u_max = max3(u_l, u_c, u_r);
  double slope;
  if ((sigma_l * sigma_r) > 0.0) slope = fsign(min2(fabs(sigma_c), 2. * min2(u_c - u_min, u_max - u_c)), sigma_c);
  else slope = 0.0;
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
    slp = min2(slp, fabs(edge - u_c) * almost_two);
  }
  edge = u_c + 0.5 * s_c;
  if ((edge - u_c) * (e_l - edge) < 0.) {
    edge = 0.5 * (edge + e_l);
    slp = min2(slp, fabs(edge - u_c) * almost_two);
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

// PLM_reconstruction :190-260 (slp, mslp: work of n values each)
__device__ void plm_reconstruction(int n, const double *h, const double *u, double *E, double *coef, double h_neglect, double *slp,
                                   double *mslp) {
  const double almost_one = 1. - DBL_EPSILON;
  for (int k = 1; k < n - 1; k++) slp[k] = plm_slope_wa(h[k - 1], h[k], h[k + 1], h_neglect, u[k - 1], u[k], u[k + 1]);
  slp[0] = 0.; slp[n - 1] = 0.;
  for (int k = 1; k < n - 1; k++) mslp[k] = plm_monotonized_slope(u[k - 1], u[k], u[k + 1], slp[k - 1], slp[k], slp[k + 1]);
  mslp[0] = 0.; mslp[n - 1] = 0.;
  E_(0, 0) = u[0]; E_(0, 1) = u[0]; C_(0, 0) = u[0]; C_(0, 1) = 0.;
  for (int k = 1; k < n - 1; k++) {
    const double slope = mslp[k];
    const double u_l = u[k] - 0.5 * slope;
    const double u_r = u[k] + 0.5 * slope;
    E_(k, 0) = u_l; E_(k, 1) = u_r;
    C_(k, 0) = u_l;
    C_(k, 1) = (u_r - u_l);
    const double edge = C_(k, 1) + C_(k, 0);
    const double e_r = u[k + 1] - 0.5 * fsign(mslp[k + 1], slp[k + 1]);
    if ((edge - u[k]) * (e_r - edge) < 0.) C_(k, 1) = C_(k, 1) * almost_one;
  }
  E_(n - 1, 0) = u[n - 1]; E_(n - 1, 1) = u[n - 1]; C_(n - 1, 0) = u[n - 1]; C_(n - 1, 1) = 0.;
}

// PLM_boundary_extrapolation :272-307
__device__ void plm_boundary_extrapolation(int n, const double *h, const double *u, double *E, double *coef, double h_neglect) {
  double slope = -plm_extrapolate_slope(h[1], h[0], h_neglect, u[1], u[0]);
  E_(0, 0) = u[0] - 0.5 * slope;
  E_(0, 1) = u[0] + 0.5 * slope;
  C_(0, 0) = E_(0, 0);
  C_(0, 1) = E_(0, 1) - E_(0, 0);
  slope = plm_extrapolate_slope(h[n - 2], h[n - 1], h_neglect, u[n - 2], u[n - 1]);
  E_(n - 1, 0) = u[n - 1] - 0.5 * slope;
  E_(n - 1, 1) = u[n - 1] + 0.5 * slope;
  C_(n - 1, 0) = E_(n - 1, 0);
  C_(n - 1, 1) = E_(n - 1, 1) - E_(n - 1, 0);
}

// bound_edge_values (answer_date >= 20190101), src/ALE/regrid_edge_values.F90:44-110
__device__ void bound_edge_values(int n, const double *h, const double *u, double *E) {
  for (int k = 0; k < n; k++) {
    const int km1 = (k - 1 > 0) ? k - 1 : 0, kp1 = (k + 1 < n - 1) ? k + 1 : n - 1;
    double slope_x_h = 0.0;
    if (((h[km1] + h[kp1]) + 2.0 * h[k]) > 0.0) {
      const double sigma_l = (u[k] - u[km1]);
      const double sigma_c = (u[kp1] - u[km1]) * (h[k] / ((h[km1] + h[kp1]) + 2.0 * h[k]));
      const double sigma_r = (u[kp1] - u[k]);
      if ((sigma_l * sigma_r) > 0.0) slope_x_h = fsign(min3(fabs(sigma_l), fabs(sigma_c), fabs(sigma_r)), sigma_c);
    }
    if ((u[km1] - E_(k, 0)) * (E_(k, 0) - u[k]) < 0.0) E_(k, 0) = u[k] - fsign(min2(fabs(slope_x_h), fabs(E_(k, 0) - u[k])), slope_x_h);
    if ((u[kp1] - E_(k, 1)) * (E_(k, 1) - u[k]) < 0.0) E_(k, 1) = u[k] + fsign(min2(fabs(slope_x_h), fabs(E_(k, 1) - u[k])), slope_x_h);
    E_(k, 0) = max2(min2(E_(k, 0), max2(u[km1], u[k])), min2(u[km1], u[k]));
    E_(k, 1) = max2(min2(E_(k, 1), max2(u[kp1], u[k])), min2(u[kp1], u[k]));
  }
}

// check_discontinuous_edge_values :141-159
__device__ void check_discontinuous_edge_values(int n, const double *u, double *E) {
  for (int k = 0; k < n - 1; k++) {
    if ((E_(k + 1, 0) - E_(k, 1)) * (u[k + 1] - u[k]) < 0.0) {
      double u0_avg = 0.5 * (E_(k, 1) + E_(k + 1, 0));
      u0_avg = max2(min2(u0_avg, max2(u[k], u[k + 1])), min2(u[k], u[k + 1]));
      E_(k, 1) = u0_avg;
      E_(k + 1, 0) = u0_avg;
    }
  }
}

// end_value_h4 :658-771
__device__ void end_value_h4(const double dz[4], const double u[4], double Csys[4]) {
  const double min_frac = 1.0e-6;
  double Wt[3][4];
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
  Wt[0][0] = -h1 * (I_h1234 + I_h123 + I_h12);
  Wt[1][0] = h1 * h12 * (I_h234 * I_h1234 + I_h23 * (I_h234 + I_h123));
  Wt[2][0] = -h1 * h12 * h123 * I_denom;
  Wt[0][1] = 2.0 * (I_h12 * (1.0 + (h1 + h12) * (I_h1234 + I_h123)) + h1 * I_h1234 * I_h123);
  Wt[1][1] = -2.0 * ((h1 * h12 * I_h1234) * (I_h23 * (I_h234 + I_h123)) + (h1 + h12) * (I_h1234 * I_h234 + I_h23 * (I_h234 + I_h123)));
  Wt[2][1] = 2.0 * ((h1 + h12) * h123 + h1 * h12) * I_denom;
  Wt[0][2] = -3.0 * I_h12 * I_h123 * (1.0 + I_h1234 * ((h1 + h12) + h123));
  Wt[1][2] = 3.0 * I_h23 * (I_h123 + I_h1234 * ((h1 + h12) + h123) * (I_h123 + I_h234));
  Wt[2][2] = -3.0 * ((h1 + h12) + h123) * I_denom;
  Wt[0][3] = 4.0 * I_h1234 * I_h123 * I_h12;
  Wt[1][3] = -4.0 * I_h1234 * (I_h23 * (I_h123 + I_h234));
  Wt[2][3] = 4.0 * I_denom;
  Csys[0] = ((u[0] + Wt[0][0] * (u[1] - u[0])) + Wt[1][0] * (u[2] - u[1])) + Wt[2][0] * (u[3] - u[2]);
  Csys[1] = (Wt[0][1] * (u[1] - u[0]) + Wt[1][1] * (u[2] - u[1])) + Wt[2][1] * (u[3] - u[2]);
  Csys[2] = (Wt[0][2] * (u[1] - u[0]) + Wt[1][2] * (u[2] - u[1])) + Wt[2][2] * (u[3] - u[2]);
  Csys[3] = (Wt[0][3] * (u[1] - u[0]) + Wt[1][3] * (u[2] - u[1])) + Wt[2][3] * (u[3] - u[2]);
}

__device__ void end_values_h4(int n, const double *h, const double *u, double hNeglect, double &top, double &top_r, double &bot,
                              double &bot_l) {
  double dz[4], ut[4], C[4];
  for (int i = 0; i < 4; i++) { dz[i] = max2(hNeglect, h[i]); ut[i] = u[i]; }
  end_value_h4(dz, ut, C);
  top = C[0]; top_r = C[0] + dz[0] * (C[1] + dz[0] * (C[2] + dz[0] * C[3]));
  for (int i = 0; i < 4; i++) { dz[i] = max2(hNeglect, h[n - 1 - i]); ut[i] = u[n - 1 - i]; }
  end_value_h4(dz, ut, C);
  bot = C[0]; bot_l = C[0] + dz[0] * (C[1] + dz[0] * (C[2] + dz[0] * C[3]));
}

// edge_values_explicit_h4 (answer_date >= 20190101) :222-363, n >= 4
__device__ void edge_values_explicit_h4(int n, const double *h, const double *u, double *E, double hNeglect) {
  const double hMinFrac = 1.e-5;
  for (int i = 2; i <= n - 2; i++) {
    double h0 = h[i - 2], h1 = h[i - 1], h2 = h[i], h3 = h[i + 1];
    if (h0 + h1 == 0.0 || h1 + h2 == 0.0 || h2 + h3 == 0.0) {
      const double h_min = hMinFrac * max2(hNeglect, (h0 + h1) + (h2 + h3));
      h0 = max2(h_min, h[i - 2]);
      h1 = max2(h_min, h[i - 1]);
      h2 = max2(h_min, h[i]);
      h3 = max2(h_min, h[i + 1]);
    }
    const double I_h12 = 1.0 / (h1 + h2);
    const double I_den_et2 = 1.0 / (((h0 + h1) + h2) * (h0 + h1)); const double I_h012 = (h0 + h1) * I_den_et2;
    const double I_den_et3 = 1.0 / ((h1 + (h2 + h3)) * (h2 + h3)); const double I_h123 = (h2 + h3) * I_den_et3;
    const double et1 = (1.0 + (h1 * I_h012 + (h0 + h1) * I_h123)) * I_h12 * (h2 * (h2 + h3)) * u[i - 1] +
                       (1.0 + (h2 * I_h123 + (h2 + h3) * I_h012)) * I_h12 * (h1 * (h0 + h1)) * u[i];
    const double et2 = (h1 * (h2 * (h2 + h3)) * I_den_et2) * (u[i - 1] - u[i - 2]);
    const double et3 = (h2 * (h1 * (h0 + h1)) * I_den_et3) * (u[i] - u[i + 1]);
    E_(i, 0) = (et1 + (et2 + et3)) / ((h0 + h1) + (h2 + h3));
    E_(i - 1, 1) = E_(i, 0);
  }
  double t, tr, b, bl;
  end_values_h4(n, h, u, hNeglect, t, tr, b, bl);
  E_(0, 0) = t; E_(0, 1) = tr; E_(1, 0) = E_(0, 1);
  E_(n - 1, 1) = b; E_(n - 1, 0) = bl; E_(n - 2, 1) = E_(n - 1, 0);
}

// edge_values_implicit_h4 (answer_date >= 20190101) :491-654 with solve_diag_dominant_tridiag (regrid_solvers.F90:246-280), n >= 4;
// w: work of 6 (n + 1) values
__device__ void edge_values_implicit_h4(int n, const double *h, const double *u, double *E, double hNeglect, double *w) {
  const int m = n + 1;
  double *tri_l = w, *tri_c = w + m, *tri_u = tri_c + m, *tri_b = tri_u + m, *tri_x = tri_b + m, *c1 = tri_x + m;
  for (int i = 0; i < 6 * m; i++) w[i] = 0.0;
  for (int i = 0; i < n - 1; i++) {
    double h0 = max2(h[i], hNeglect);
    double h1 = max2(h[i + 1], hNeglect);
    if (fabs(h0) < 1.0e-12 * fabs(h1)) h0 = 1.0e-12 * h1;
    if (fabs(h1) < 1.0e-12 * fabs(h0)) h1 = 1.0e-12 * h0;
    const double I_h2 = 1.0 / ((h0 + h1) * (h0 + h1));
    const double alpha = (h1 * h1) * I_h2;
    const double beta = (h0 * h0) * I_h2;
    const double abmix = (h0 * h1) * I_h2;
    const double a = 2.0 * alpha * (alpha + 2.0 * beta + 3.0 * abmix);
    const double b = 2.0 * beta * (beta + 2.0 * alpha + 3.0 * abmix);
    tri_c[i + 1] = 2.0 * abmix;
    tri_l[i + 1] = alpha;
    tri_u[i + 1] = beta;
    tri_b[i + 1] = a * u[i] + b * u[i + 1];
  }
  double t, tr, bt, bl;
  end_values_h4(n, h, u, hNeglect, t, tr, bt, bl);
  tri_b[0] = t; tri_c[0] = 1.0; tri_u[0] = 0.0;
  tri_b[n] = bt; tri_c[n] = 1.0; tri_l[n] = 0.0;
  double I_pivot = 1.0 / (tri_c[0] + tri_u[0]);
  double d1 = tri_c[0] * I_pivot;
  c1[0] = tri_u[0] * I_pivot;
  tri_x[0] = tri_b[0] * I_pivot;
  for (int k = 1; k < m - 1; k++) {
    const double denom_t1 = tri_c[k] + d1 * tri_l[k];
    I_pivot = 1.0 / (denom_t1 + tri_u[k]);
    d1 = denom_t1 * I_pivot;
    c1[k] = tri_u[k] * I_pivot;
    tri_x[k] = (tri_b[k] - tri_l[k] * tri_x[k - 1]) * I_pivot;
  }
  I_pivot = 1.0 / (tri_c[m - 1] + d1 * tri_l[m - 1]);
  tri_x[m - 1] = (tri_b[m - 1] - tri_l[m - 1] * tri_x[m - 2]) * I_pivot;
  for (int k = m - 2; k >= 0; k--) tri_x[k] = tri_x[k] - c1[k] * tri_x[k + 1];
  E_(0, 0) = tri_x[0];
  for (int i = 1; i < n; i++) { E_(i, 0) = tri_x[i]; E_(i - 1, 1) = tri_x[i]; }
  E_(n - 1, 1) = tri_x[n];
}

// edge_values_explicit_h4cw :381-470, n >= 4; w: work of 8 (n + 2) values (1-based as in the reference)
__device__ void edge_values_explicit_h4cw(int n, const double *h, const double *u, double *E, double hNeglect, double *w) {
  const int m = n + 2;
  double *dp = w, *au = dp + m, *al = au + m, *ar = al + m, *h112 = ar + m, *h122 = h112 + m, *I_h12 = h122 + m, *h2_h123 = I_h12 + m;
  for (int i = 0; i < 8 * m; i++) w[i] = 0.0;
#define U1(k) u[(k) - 1]
  for (int k = 1; k <= n; k++) dp[k] = max2(h[k - 1], hNeglect);
  for (int k = 2; k <= n; k++) {
    h112[k] = 2. * dp[k - 1] + dp[k];
    h122[k] = dp[k - 1] + 2. * dp[k];
    I_h12[k] = 1.0 / (dp[k - 1] + dp[k]);
  }
  for (int k = 2; k <= n - 1; k++) h2_h123[k] = dp[k] / (dp[k] + (dp[k - 1] + dp[k + 1]));
  au[1] = 0.;
  for (int k = 2; k <= n - 1; k++) {
    const double slk = U1(k) - U1(k - 1);
    const double srk = U1(k + 1) - U1(k);
    if (slk * srk > 0.) {
      const double sck = h2_h123[k] * (h112[k] * srk * I_h12[k + 1] + h122[k + 1] * slk * I_h12[k]);
      au[k] = fsign(min3(fabs(2.0 * slk), fabs(sck), fabs(2.0 * srk)), sck);
    } else {
      au[k] = 0.;
    }
  }
  au[n] = 0.;
  al[1] = U1(1); ar[1] = U1(1); al[2] = U1(1);
  for (int k = 3; k <= n - 1; k++) {
    const double I_h0123 = 1.0 / ((dp[k - 2] + dp[k - 1]) + (dp[k] + dp[k + 1]));
    const double h01_h112 = (dp[k - 2] + dp[k - 1]) / (2.0 * dp[k - 1] + dp[k]);
    const double h23_h122 = (dp[k] + dp[k + 1]) / (dp[k - 1] + 2.0 * dp[k]);
    al[k] = (dp[k] * U1(k - 1) + dp[k - 1] * U1(k)) * I_h12[k] +
            I_h0123 * (2. * dp[k] * dp[k - 1] * I_h12[k] * (U1(k) - U1(k - 1)) * (h01_h112 - h23_h122) +
                       (dp[k] * au[k - 1] * h23_h122 - dp[k - 1] * au[k] * h01_h112));
    ar[k - 1] = al[k];
  }
  ar[n - 1] = U1(n); al[n] = U1(n); ar[n] = U1(n);
  for (int k = 1; k <= n; k++) { E_(k - 1, 0) = al[k]; E_(k - 1, 1) = ar[k]; }
#undef U1
}

// PPM_monotonicity, src/ALE/PPM_functions.F90:132-158
__device__ void ppm_monotonicity(int n, const double *u, double *E) {
  for (int k = 1; k < n - 1; k++) {
    if ((u[k + 1] - u[k]) * (u[k] - u[k - 1]) <= 0.) {
      E_(k, 0) = u[k];
      E_(k, 1) = u[k];
    } else {
      const double da = E_(k, 1) - E_(k, 0);
      const double a6 = 6.0 * u[k] - 3.0 * (E_(k, 0) + E_(k, 1));
      if (da * a6 > da * da) E_(k, 0) = 3.0 * u[k] - 2.0 * E_(k, 1);
      else if (da * a6 < -da * da) E_(k, 1) = 3.0 * u[k] - 2.0 * E_(k, 0);
    }
  }
}

// PPM_reconstruction with PPM_limiter_standard :28-128
__device__ void ppm_reconstruction(int n, const double *h, const double *u, double *E, double *coef) {
  bound_edge_values(n, h, u, E);
  check_discontinuous_edge_values(n, u, E);
  for (int k = 1; k < n - 1; k++) {
    const double u_l = u[k - 1], u_c = u[k], u_r = u[k + 1];
    double edge_l = E_(k, 0), edge_r = E_(k, 1);
    if ((u_r - u_c) * (u_c - u_l) <= 0.0) {
      edge_l = u_c; edge_r = u_c;
    } else {
      const double expr1 = 3.0 * (edge_r - edge_l) * ((u_c - edge_l) + (u_c - edge_r));
      const double expr2 = (edge_r - edge_l) * (edge_r - edge_l);
      if (expr1 > expr2) {
        edge_l = u_c + 2.0 * (u_c - edge_r);
        edge_l = max2(min2(edge_l, max2(u_l, u_c)), min2(u_l, u_c));
      } else if (expr1 < -expr2) {
        edge_r = u_c + 2.0 * (u_c - edge_l);
        edge_r = max2(min2(edge_r, max2(u_r, u_c)), min2(u_r, u_c));
      }
    }
    if (fabs(edge_r - edge_l) < max2(1.e-60, DBL_EPSILON * fabs(u_c))) { edge_l = u_c; edge_r = u_c; }
    E_(k, 0) = edge_l; E_(k, 1) = edge_r;
  }
  E_(0, 0) = u[0]; E_(0, 1) = u[0];
  E_(n - 1, 0) = u[n - 1]; E_(n - 1, 1) = u[n - 1];
  for (int k = 0; k < n; k++) {
    const double edge_l = E_(k, 0), edge_r = E_(k, 1);
    C_(k, 0) = edge_l;
    C_(k, 1) = 4.0 * (u[k] - edge_l) + 2.0 * (u[k] - edge_r);
    C_(k, 2) = 3.0 * ((edge_r - u[k]) + (edge_l - u[k]));
  }
}

// PPM_boundary_extrapolation :162-316
__device__ void ppm_boundary_extrapolation(int n, const double *h, const double *u, double *E, double *coef, double hNeglect) {
  int i0 = 0, i1 = 1;
  double h0 = h[i0], h1 = h[i1], u0 = u[i0], u1 = u[i1];
  double b = C_(i1, 1);
  double u1_r = b * ((h0 + hNeglect) / (h1 + hNeglect));
  double slope = 2.0 * (u1 - u0);
  if (fabs(u1_r) > fabs(slope)) u1_r = slope;
  double u0_r = E_(i1, 0);
  double u0_l = 3.0 * u0 + 0.5 * u1_r - 2.0 * u0_r;
  double exp1 = (u0_r - u0_l) * (u0 - 0.5 * (u0_l + u0_r));
  double exp2 = (u0_r - u0_l) * (u0_r - u0_l) / 6.0;
  if (exp1 > exp2) u0_l = 3.0 * u0 - 2.0 * u0_r;
  if (exp1 < -exp2) u0_r = 3.0 * u0 - 2.0 * u0_l;
  E_(i0, 0) = u0_l; E_(i0, 1) = u0_r;
  C_(i0, 0) = u0_l;
  C_(i0, 1) = 6.0 * u0 - 4.0 * u0_l - 2.0 * u0_r;
  C_(i0, 2) = 3.0 * (u0_r + u0_l - 2.0 * u0);

  i0 = n - 2; i1 = n - 1;
  h0 = h[i0]; h1 = h[i1]; u0 = u[i0]; u1 = u[i1];
  b = C_(i0, 1);
  const double c = C_(i0, 2);
  double u1_l = (b + 2 * c);
  u1_l = u1_l * ((h1 + hNeglect) / (h0 + hNeglect));
  slope = 2.0 * (u1 - u0);
  if (fabs(u1_l) > fabs(slope)) u1_l = slope;
  u0_l = E_(i0, 1);
  u0_r = 3.0 * u1 - 0.5 * u1_l - 2.0 * u0_l;
  exp1 = (u0_r - u0_l) * (u1 - 0.5 * (u0_l + u0_r));
  exp2 = (u0_r - u0_l) * (u0_r - u0_l) / 6.0;
  if (exp1 > exp2) u0_l = 3.0 * u1 - 2.0 * u0_r;
  if (exp1 < -exp2) u0_r = 3.0 * u1 - 2.0 * u0_l;
  E_(i1, 0) = u0_l; E_(i1, 1) = u0_r;
  C_(i1, 0) = u0_l;
  C_(i1, 1) = 6.0 * u1 - 4.0 * u0_l - 2.0 * u0_r;
  C_(i1, 2) = 3.0 * (u0_r + u0_l - 2.0 * u1);
}

// average_value_ppoly, src/ALE/MOM_remapping.F90:998-1099 (PCM, PLM, PPM)
__device__ double average_value_ppoly(int n, const double *u0, const double *E, const double *coef, int method, int i0, double xa, double xb) {
  double u_ave = 0.0;
  if (xb > xa) {
    if (method == INT_PCM) {
      u_ave = u0[i0];
    } else if (method == INT_PLM) {
      u_ave = (C_(i0, 0) + C_(i0, 1) * 0.5 * (xb + xa));
    } else {
      const double mx = 0.5 * (xa + xb);
      const double a_L = E_(i0, 0), a_R = E_(i0, 1), u_c = u0[i0];
      const double a_c = 0.5 * ((u_c - a_L) + (u_c - a_R));
      if (mx < 0.5) {
        const double xa2b2ab = (xa * xa + xb * xb) + xa * xb;
        u_ave = a_L + ((a_R - a_L) * mx + a_c * (3. * (xb + xa) - 2. * xa2b2ab));
      } else {
        const double Ya = 1. - xa, Yb = 1. - xb;
        const double my = 0.5 * (Ya + Yb);
        const double Ya2b2ab = (Ya * Ya + Yb * Yb) + Ya * Yb;
        u_ave = a_R + ((a_L - a_R) * my + a_c * (3. * (Yb + Ya) - 2. * Ya2b2ab));
      }
    }
  } else {
    if (method == INT_PCM) {
      u_ave = C_(i0, 0);
    } else if (method == INT_PLM) {
      const double a_L = E_(i0, 0), a_R = E_(i0, 1);
      const double Ya = 1. - xa;
      if (xa < 0.5) u_ave = a_L + xa * (a_R - a_L);
      else u_ave = a_R + Ya * (a_L - a_R);
    } else {
      const double a_L = E_(i0, 0), a_R = E_(i0, 1), u_c = u0[i0];
      const double a_c = 3. * ((u_c - a_L) + (u_c - a_R));
      const double Ya = 1. - xa;
      if (xa < 0.5) u_ave = a_L + xa * ((a_R - a_L) + a_c * Ya);
      else u_ave = a_R + Ya * ((a_L - a_R) + a_c * xa);
    }
  }
  return u_ave;
}
#undef E_
#undef C_

// the private work space of one remapping_core_h of at most NKM source and 2 NKM + 2 target cells
template <int NKM>
struct RemapWork {
  static constexpr int N1M = 2 * NKM + 2, NS = NKM + N1M + 3;
  double E[2 * NKM], coef[3 * NKM], w[8 * (NKM + 2)];
  double h_sub[NS], uh_sub[NS], u_sub[NS], h0_eff[NKM + 2];
  int isub_src[NS], isrc_start[NKM + 2], isrc_end[NKM + 2], isrc_max[NKM + 2], itgt_start[N1M + 2], itgt_end[N1M + 2];
};

// build_reconstructions_1d (:257-386) for the schemes provided; returns the integration method
template <int NKM>
__device__ int build_reconstructions(RemapWork<NKM> &W, int scheme, bool extrap, int n0, const double *h0, const double *u0,
                                     double h_neglect, double h_neglect_edge) {
  const int n = n0;
  for (int i = 0; i < 2 * n0; i++) W.E[i] = 0.0;
  for (int i = 0; i < 3 * n0; i++) W.coef[i] = 0.0;
  int local = scheme;
  if (n0 <= 1) local = MOM6HIP_REMAP_PCM;
  else if (n0 <= 3) local = (local < MOM6HIP_REMAP_PLM) ? local : MOM6HIP_REMAP_PLM;
  else if (n0 <= 4 && local != MOM6HIP_REMAP_PPM_CW) local = (local < MOM6HIP_REMAP_PPM_H4) ? local : MOM6HIP_REMAP_PPM_H4;
  if (local == MOM6HIP_REMAP_PCM) {
    for (int k = 0; k < n; k++) { W.coef[k] = u0[k]; W.E[k] = u0[k]; W.E[n + k] = u0[k]; }
    return INT_PCM;
  }
  if (local == MOM6HIP_REMAP_PLM) {
    plm_reconstruction(n, h0, u0, W.E, W.coef, h_neglect, W.w, W.w + n);
    if (extrap) plm_boundary_extrapolation(n, h0, u0, W.E, W.coef, h_neglect);
    return INT_PLM;
  }
  if (local == MOM6HIP_REMAP_PPM_H4) edge_values_explicit_h4(n, h0, u0, W.E, h_neglect_edge);
  else if (local == MOM6HIP_REMAP_PPM_IH4) edge_values_implicit_h4(n, h0, u0, W.E, h_neglect_edge, W.w);
  else { edge_values_explicit_h4cw(n, h0, u0, W.E, h_neglect_edge, W.w); ppm_monotonicity(n, u0, W.E); }
  ppm_reconstruction(n, h0, u0, W.E, W.coef);
  if (extrap) ppm_boundary_extrapolation(n, h0, u0, W.E, W.coef, h_neglect);
  return INT_PPM;
}

// remap_via_sub_cells (:463-852) with force_bounds_in_subcell = .false. (n1 >= 1)
template <int NKM>
__device__ void remap_via_sub_cells(RemapWork<NKM> &W, int n0, const double *h0, const double *u0, int n1, const double *h1, int method,
                                    double *u1) {
  const int n = n0, ns = n0 + n1 + 1;
  const double *E = W.E;
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
  u_sub[1] = E[0];
  for (int i_sub = 2; i_sub <= n0 + n1; i_sub++) {
    dh = h_sub[i_sub];
    i0 = isub_src[i_sub];
    dh0_eff = dh0_eff + dh;
    if (h0_eff[i0] > 0.) {
      xb = dh0_eff / h0_eff[i0];
      xb = min2(1., xb);
      u_sub[i_sub] = average_value_ppoly(n0, u0, E, W.coef, method, i0 - 1, xa, xb);
    } else {
      xb = 1.;
      u_sub[i_sub] = U0(i0);
    }
    uh_sub[i_sub] = dh * u_sub[i_sub];
    if (isub_src[i_sub + 1] != i0) { dh0_eff = 0.; xa = 0.; }
    else { xa = xb; }
  }
  u_sub[ns] = E[n + n0 - 1];
  uh_sub[ns] = E[n + n0 - 1] * h_sub[ns];
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

// boundary_k_range(SURFACE, ...) :609-647: k_bot (1-based); h is a plane-strided column of nk values
__device__ int boundary_k_bot(int nk, const double *h, long stride, double hbl) {
  if (hbl == 0.) return 1;
  double hsum = 0.;
  for (int k = 0; k < nk; k++) hsum = hsum + h[stride * k];
  if (hbl >= hsum) return nk;
  double htot = 0.;
  for (int k = 0; k < nk; k++) {
    htot = htot + h[stride * k];
    if (htot >= hbl) return k + 1;
  }
  return 1;
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
  const int k_bot_L = boundary_k_bot(km, dz, 1, hbl_L), k_bot_R = boundary_k_bot(km, dz, 1, hbl_R);
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

// thread (i, j, k) over the compute domain
__global__ __launch_bounds__(256) void hbd_update_kernel(HBDArgs A) {
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
  }
  if (A.cu > 0.0 && fabs(x) < A.cu) x = 0.0;
  A.t[n] = x;
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
// khdt_x at every interface, each after a group pass of the tracers.  h, h_ML, khdt_x / khdt_y and the tracers are device arrays.
// ebt_struct is VarMix%ebt_struct with KHTR_USE_EBT_STRUCT and null without.
int hbd_branch(mom6hip_ctx_t *ctx, Stager &st, const mom6hip_hor_bnd_diffusion_cs_t *hbd, const double *h, const double *h_ML,
               const double *ebt_struct, double KhTr_min, bool full_depth_khtr_min, const double *khdt_x, const double *khdt_y, int num_itts,
               double I_numitts, const std::vector<double *> &d_tr, const std::vector<double> &cu, int *halo_updates) {
  M6_REQUIRE(hbd->initialized, "hor_bnd_diffusion: the control structure is not initialised");
  M6_REQUIRE(!hbd->debug, "hor_bnd_diffusion: HBD_DEBUG is not provided by libmom6hip");
  M6_REQUIRE(!hbd->diagnostics, "hor_bnd_diffusion: the hbd_* diagnostics are not provided by libmom6hip");
  M6_REQUIRE(hbd_scheme_provided(hbd->remap_scheme), "hor_bnd_diffusion: HBD_REMAPPING_SCHEME %d is not provided by libmom6hip "
             "(PCM, PLM, PPM_H4, PPM_IH4 and PPM_CW are)", hbd->remap_scheme);
  M6_REQUIRE(h_ML != nullptr, "hor_bnd_diffusion requires that visc%%h_ML is associated.");
  const m6::GridDev g = ctx->g;
  M6_REQUIRE(g.mask2dT && g.mask2dCu && g.mask2dCv && g.areaT && g.IareaT, "hor_bnd_diffusion: mask2dT, mask2dCu, mask2dCv, areaT and IareaT are needed");
  M6_REQUIRE(g.nk >= 1 && g.nk <= 128, "hor_bnd_diffusion: 1 to 128 layers are supported");
  hipStream_t s = ctx->stream;
  const int ntr = (int)d_tr.size(), nk = g.nk;
  const size_t hpl = (size_t)g.nih * g.njh, upl = (size_t)(g.nih + 1) * g.njh, vpl = (size_t)g.nih * (g.njh + 1);
  HBDArgs A;
  A.g = g; A.h = h; A.khdt[0] = khdt_x; A.khdt[1] = khdt_y; A.I_numitts = I_numitts; A.h_neglect = g.H_subroundoff;
  A.linear = hbd->linear; A.limiter = hbd->limiter; A.limiter_remap = hbd->limiter_remap; A.extrap = hbd->boundary_extrap;
  A.scheme = hbd->remap_scheme; A.t = nullptr; A.cu = 0.0;
  A.ebt = ebt_struct; A.KhTr_min = KhTr_min; A.full_depth_khtr_min = full_depth_khtr_min ? 1 : 0;
  double *hbl = (double *)st.scratch(sizeof(double) * hpl);
  A.kmax[0] = (int *)st.scratch(sizeof(int) * upl); A.nflx[0] = (int *)st.scratch(sizeof(int) * upl);
  A.kmax[1] = (int *)st.scratch(sizeof(int) * vpl); A.nflx[1] = (int *)st.scratch(sizeof(int) * vpl);
  A.maxes = (int *)st.scratch(64);
  M6_REQUIRE(!st.failed() && hbl && A.kmax[0] && A.nflx[0] && A.kmax[1] && A.nflx[1] && A.maxes, "hor_bnd_diffusion: out of device memory");
  A.hbl = hbl;
  // hbl = visc%h_ML; pass_var(hbl, halo=1) (:217-222).  h and hbl do not change between the calls: the HBD grid is built once.
  M6_HIP(hipMemcpyAsync(hbl, h_ML, sizeof(double) * hpl, hipMemcpyDeviceToDevice, s));
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
  for (int itt = 1; itt <= num_itts; itt++) {
    if (int rc = m6::group_pass(ctx, pf.data(), ppos.data(), pnk.data(), ntr)) return rc;      // :412, and :466 for itt > 1
    (*halo_updates)++;
    for (int m = 0; m < ntr; m++) {
      A.t = d_tr[m]; A.cu = cu[m];
      if (A.nflx_max[0] + A.nflx_max[1] > 0) {
        if (nkm == 16) launch_flux<16>(A, nbu, nj, nbv, nj + 1, s);
        else if (nkm == 80) launch_flux<80>(A, nbu, nj, nbv, nj + 1, s);
        else launch_flux<128>(A, nbu, nj, nbv, nj + 1, s);
      }
      hipLaunchKernelGGL(hbd_update_kernel, dim3((ni + 255) / 256, nj, nk), dim3(256), 0, s, A);
    }
  }
  M6_HIP(hipGetLastError());
  return 0;
}

}  // namespace m6

extern "C" uint64_t mom6hip_abi_sizeof_hor_bnd_diffusion_cs(void) { return sizeof(mom6hip_hor_bnd_diffusion_cs_t); }
