// flux_diag_march.hpp -- the ordered march over the layers that the tracer flux diagnostics of advect_tracer (tracer_advect.hip) and of
// tracer_hordiff (tracer_hor_diff.hip) share.  The marching kernels of a pass, or the step kernel of an iteration, leave the increment of
// every face and layer (flux * Idt) in face-shaped scratch; flux_diag_march_kernel then runs a thread a face (lanes along i, so every load
// is i-contiguous), which walks k = 1..nz and adds the increments to the 3-D array and, in that order of k, to the 2-D array: the
// reference sums ad2d_x / ad2d_y (MOM_tracer_advect.F90:689-698, :1078-1084) and df2d_x / df2d_y (MOM_tracer_hor_diff.F90:584-591) layer by
// layer, and the order is part of the answer -- no atomics, no tree.
#pragma once

#include "common.hpp"

namespace m6 {

constexpr int FLUX_DIAG_MAXD = 8;      // tracers a launch of the march takes

struct FluxDiagMarch {
  GridDev g;
  const double *face[FLUX_DIAG_MAXD];      // the increments, face-shaped with nk layers
  double *a3[FLUX_DIAG_MAXD], *a2[FLUX_DIAG_MAXD];      // the 3-D and the 2-D array (null: not asked for)
  const int *doi;          // h-shaped, nk layers: a layer of a face counts where either of its two cells is set (null: every face counts)
  int skip0, skip1;        // the layers skip0 <= k < skip1 (0-based) take no part (an empty range: every layer does)
  int zero;                // 1: no increments; the arrays are set to zero over the range instead
  int n, is, ie, js, je;   // the faces: I = is-1..ie, j = js..je (DIR 0) | i = is..ie, J = js-1..je (DIR 1)
};

template <int DIR>
__global__ __launch_bounds__(256) void flux_diag_march_kernel(FluxDiagMarch a) {
  const GridDev &g = a.g;
  const int tx = blockIdx.x * 256 + threadIdx.x;
  const int i = (DIR ? a.is : a.is - 1) + tx, j = (DIR ? a.js - 1 : a.js) + (int)blockIdx.y;      // the face (I, j) | (i, J)
  if (i > a.ie) return;
  const FaceCol<DIR> fc(g, i, j);
  if (a.zero) {
    for (int n = 0; n < a.n; n++) {
      if (a.a3[n]) for (int k = 0; k < g.nk; k++) a.a3[n][fc.f2 + fc.fpl * k] = 0.0;
      if (a.a2[n]) a.a2[n][fc.f2] = 0.0;
    }
    return;
  }
  double acc[FLUX_DIAG_MAXD];
#pragma unroll
  for (int n = 0; n < FLUX_DIAG_MAXD; n++) acc[n] = (n < a.n && a.a2[n]) ? a.a2[n][fc.f2] : 0.0;
  for (int k = 0; k < g.nk; k++) {
    if (k >= a.skip0 && k < a.skip1) continue;
    if (a.doi && !(a.doi[fc.c0 + fc.hpl * k] | a.doi[fc.c1 + fc.hpl * k])) continue;
    const long f3 = fc.f2 + fc.fpl * k;
#pragma unroll
    for (int n = 0; n < FLUX_DIAG_MAXD; n++) if (n < a.n) {
      const double v = a.face[n][f3];
      if (a.a3[n]) a.a3[n][f3] = a.a3[n][f3] + v;
      acc[n] = acc[n] + v;
    }
  }
#pragma unroll
  for (int n = 0; n < FLUX_DIAG_MAXD; n++) if (n < a.n && a.a2[n]) a.a2[n][fc.f2] = acc[n];
}

inline void flux_diag_march(int dir, const FluxDiagMarch &a, hipStream_t s) {
  const dim3 grid = dir ? dim3((a.ie - a.is + 1 + 255) / 256, a.je - a.js + 2) : dim3((a.ie - a.is + 2 + 255) / 256, a.je - a.js + 1);
  if (dir) hipLaunchKernelGGL(flux_diag_march_kernel<1>, grid, dim3(256), 0, s, a);
  else     hipLaunchKernelGGL(flux_diag_march_kernel<0>, grid, dim3(256), 0, s, a);
}

// The same march for cell-shaped tendencies: a2(i,j) = sum over k = 1..nz of a3(i,j,k), from 0.0 in layer order, over the compute domain
// (the depth-summed content tendencies dfxy_cont_2d, MOM_neutral_diffusion.F90:997-1004, and hbdxy_cont_2d, MOM_hor_bnd_diffusion.F90:316-323).
// One thread a column, lanes along i; up to FLUX_DIAG_MAXD tracers a launch.
struct CellSumMarch {
  GridDev g;
  const double *a3[FLUX_DIAG_MAXD];
  double *a2[FLUX_DIAG_MAXD];
  int n;
};

static __global__ __launch_bounds__(256) void cell_sum_march_kernel(CellSumMarch a) {
  const GridDev &g = a.g;
  const int i = g.isc + blockIdx.x * 256 + threadIdx.x, j = g.jsc + (int)blockIdx.y;
  if (i > g.iec) return;
  const long n2 = g.h2(i, j), hpl = (long)g.nih * g.njh;
  for (int n = 0; n < a.n; n++) {
    double acc = 0.0;
    for (int k = 0; k < g.nk; k++) acc = acc + a.a3[n][n2 + hpl * k];
    a.a2[n][n2] = acc;
  }
}

inline void cell_sum_march(const CellSumMarch &a, hipStream_t s) {
  const GridDev &g = a.g;
  hipLaunchKernelGGL(cell_sum_march_kernel, dim3((g.iec - g.isc + 1 + 255) / 256, g.jec - g.jsc + 1), dim3(256), 0, s, a);
}

}  // namespace m6
