// remap_column.hpp -- the reconstructions of one column by one lane: serial loops over the pieces of remap_pieces.hpp (PLM_reconstruction,
// the explicit and implicit h4 edge values, h4cw, bound_edge_values, check_discontinuous_edge_values, PPM_reconstruction), for the files
// whose lanes hold a column in private arrays: hor_bnd_diffusion.hip and neutral_diffusion_disc.hip.  Include remap_pieces.hpp first.
#pragma once

namespace {

using m6::max2;
using m6::min2;

// ---- the reconstructions of one column of n cells (k 0-based), serial loops over the pieces of remap_pieces.hpp ------------------------
// PLM_reconstruction :190-260 (slp, mslp: work of n values each)
__device__ void plm_reconstruction(int n, const double *h, const double *u, double *EL, double *ER, double *C1, double h_neglect,
                                   double *slp, double *mslp) {
  const double almost_one = 1. - DBL_EPSILON;
  for (int k = 1; k < n - 1; k++) slp[k] = plm_slope_wa(h[k - 1], h[k], h[k + 1], h_neglect, u[k - 1], u[k], u[k + 1]);
  slp[0] = 0.; slp[n - 1] = 0.;
  for (int k = 1; k < n - 1; k++) mslp[k] = plm_monotonized_slope(u[k - 1], u[k], u[k + 1], slp[k - 1], slp[k], slp[k + 1]);
  mslp[0] = 0.; mslp[n - 1] = 0.;
  EL[0] = u[0]; ER[0] = u[0]; C1[0] = 0.;
  for (int k = 1; k < n - 1; k++) {
    const double slope = mslp[k];
    const double u_l = u[k] - 0.5 * slope;
    const double u_r = u[k] + 0.5 * slope;
    EL[k] = u_l; ER[k] = u_r;
    double c1 = (u_r - u_l);
    const double edge = c1 + u_l;
    const double e_r = u[k + 1] - 0.5 * fsign(mslp[k + 1], slp[k + 1]);
    if ((edge - u[k]) * (e_r - edge) < 0.) c1 = c1 * almost_one;
    C1[k] = c1;
  }
  EL[n - 1] = u[n - 1]; ER[n - 1] = u[n - 1]; C1[n - 1] = 0.;
}

// bound_edge_values (answer_date >= 20190101), src/ALE/regrid_edge_values.F90:44-110
__device__ void bound_edge_values(int n, const double *h, const double *u, double *EL, double *ER) {
  for (int k = 0; k < n; k++) {
    const int km1 = (k - 1 > 0) ? k - 1 : 0, kp1 = (k + 1 < n - 1) ? k + 1 : n - 1;
    const double den = (h[km1] + h[kp1]) + 2.0 * h[k];
    const double slope_x_h = bound_slope(u[km1], u[k], u[kp1], den > 0.0 ? h[k] / den : -1.0);
    EL[k] = bound_left(EL[k], u[km1], u[k], slope_x_h);
    ER[k] = bound_right(ER[k], u[kp1], u[k], slope_x_h);
  }
}

// check_discontinuous_edge_values :141-159
__device__ void check_discontinuous_edge_values(int n, const double *u, double *EL, double *ER) {
  for (int k = 0; k < n - 1; k++) {
    if (edges_discontinuous(u[k], u[k + 1], ER[k], EL[k + 1])) {
      const double u0_avg = bounded_edge_average(u[k], u[k + 1], ER[k], EL[k + 1]);
      ER[k] = u0_avg; EL[k + 1] = u0_avg;
    }
  }
}

// edge_values_explicit_h4 (answer_date >= 20190101) :222-363, n >= 4
__device__ void edge_values_explicit_h4(int n, const double *h, const double *u, double *EL, double *ER, double hNeglect) {
  for (int i = 2; i <= n - 2; i++) {
    const EdgeW w = edge_weights_h4(h[i - 2], h[i - 1], h[i], h[i + 1], hNeglect);
    const double ev = edge_value_h4(w, u[i - 2], u[i - 1], u[i], u[i + 1]);
    EL[i] = ev; ER[i - 1] = ev;
  }
  double Cs[4];
  double dz0 = end_polynomial_h4(h, u, false, n, hNeglect, Cs);
  EL[0] = Cs[0]; ER[0] = Cs[0] + dz0 * (Cs[1] + dz0 * (Cs[2] + dz0 * Cs[3])); EL[1] = ER[0];
  dz0 = end_polynomial_h4(h, u, true, n, hNeglect, Cs);
  ER[n - 1] = Cs[0]; EL[n - 1] = Cs[0] + dz0 * (Cs[1] + dz0 * (Cs[2] + dz0 * Cs[3])); ER[n - 2] = EL[n - 1];
}

// edge_values_implicit_h4 (answer_date >= 20190101) :491-654, n >= 4; w: work of 5 (n + 1) values
__device__ void edge_values_implicit_h4(int n, const double *h, const double *u, double *EL, double *ER, double hNeglect, double *w) {
  const int m = n + 1;
  double *tri_l = w, *tri_c = w + m, *tri_u = tri_c + m, *tri_b = tri_u + m, *c1 = tri_b + m;
  for (int i = 0; i < n - 1; i++) {
    const TriRow r = implicit_h4_row(h[i], h[i + 1], u[i], u[i + 1], hNeglect);
    tri_c[i + 1] = r.c; tri_l[i + 1] = r.l; tri_u[i + 1] = r.u; tri_b[i + 1] = r.b;
  }
  double Cs[4];
  end_polynomial_h4(h, u, false, n, hNeglect, Cs);
  tri_b[0] = Cs[0]; tri_c[0] = 1.0; tri_u[0] = 0.0; tri_l[0] = 0.0;
  end_polynomial_h4(h, u, true, n, hNeglect, Cs);
  tri_b[n] = Cs[0]; tri_c[n] = 1.0; tri_u[n] = 0.0; tri_l[n] = 0.0;
  solve_diag_dominant_tridiag(tri_l, tri_c, tri_u, tri_b, c1, m);
  for (int k = 0; k < n; k++) { EL[k] = tri_b[k]; ER[k] = tri_b[k + 1]; }
}

// edge_values_explicit_h4cw :381-470 and PPM_monotonicity (PPM_functions.F90:132-158), n >= 4; au: work of n values
__device__ void edge_values_explicit_h4cw(int n, const double *h, const double *u, double *EL, double *ER, double hNeglect, double *au) {
  auto dp = [&](int k) { return max2(h[k], hNeglect); };
  au[0] = 0.; au[n - 1] = 0.;
  for (int k = 1; k <= n - 2; k++) au[k] = h4cw_slope(dp(k - 1), dp(k), dp(k + 1), u[k - 1], u[k], u[k + 1]);
  for (int k = 2; k <= n - 2; k++) {
    const double al = h4cw_edge(dp(k - 2), dp(k - 1), dp(k), dp(k + 1), u[k - 1], u[k], au[k - 1], au[k]);
    EL[k] = al; ER[k - 1] = al;
  }
  EL[0] = u[0]; ER[0] = u[0]; EL[1] = u[0]; ER[n - 2] = u[n - 1]; EL[n - 1] = u[n - 1]; ER[n - 1] = u[n - 1];
}
__device__ void ppm_monotonicity(int n, const double *u, double *EL, double *ER) {
  for (int k = 1; k < n - 1; k++) {
    double edge_l = EL[k], edge_r = ER[k];
    ppm_monotonicity_cell(u[k - 1], u[k], u[k + 1], edge_l, edge_r);
    EL[k] = edge_l; ER[k] = edge_r;
  }
}

// PPM_reconstruction with PPM_limiter_standard :28-128
__device__ void ppm_reconstruction(int n, const double *h, const double *u, double *EL, double *ER, double *C1) {
  bound_edge_values(n, h, u, EL, ER);
  check_discontinuous_edge_values(n, u, EL, ER);
  for (int k = 0; k < n; k++) {
    double edge_l = u[k], edge_r = u[k];      // the boundary cells are piecewise constant
    if (k >= 1 && k < n - 1) {
      edge_l = EL[k]; edge_r = ER[k];
      ppm_limit_cell(u[k - 1], u[k], u[k + 1], edge_l, edge_r);
    }
    EL[k] = edge_l; ER[k] = edge_r;
    C1[k] = 4.0 * (u[k] - edge_l) + 2.0 * (u[k] - edge_r);
  }
}

}  // namespace
