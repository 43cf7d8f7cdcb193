// tracer_hor_diff.hip -- tracer_hordiff (src/tracer/MOM_tracer_hor_diff.F90:119-680) as gfx950 kernels: the along-layer diffusion
// with KHTR or the VarMix / MEKE diffusivities, the call of the neutral-diffusion branch (neutral_diffusion.hip), and with
// DIFFUSE_ML_TO_INTERIOR the scaled / skipped variable-density layers (:544-550) and the call of tracer_epipycnal_ML_diff
// (epipycnal_diff.hip).
//
//   hd_khdt_kernel    khdt_x, khdt_y (:340-351), their MAX_TR_DIFFUSION_CFL limit (:368-398) and, with CHECK_DIFFUSIVE_CFL,
//                     the largest diffusive CFL number (:410-416; an atomic max on the bit pattern of positive doubles)
//   hd_step_kernel    one iteration for every tracer of a layer point: the four face coefficients (harmonic-mean
//                     thicknesses, :552-561) and Ihdxdy are formed once per point and serve all tracers; the new values go
//                     to a work copy because the reference updates a layer only after all its dTr are formed (:568-594)
//   hd_commit_kernel  work copy -> tracer on the compute domain, with the concentration underflow (:607-612)
// Every layer and point is independent: thread per point, lanes along i, blockIdx.z = k.
// Algorithmic traffic per iteration: read h, read and write every tracer = 8 + 16 ntr B per cell (the work copy doubles the
// tracer part).
#include <cfloat>
#include <array>
#include <cmath>
#include <type_traits>

#include "flux_diag_march.hpp"
#include "hordiff_call.hpp"

namespace {

using m6::min2;

using m6::max2;

struct HDArgs {
  m6::GridDev g;
  double KhTr, max_diff_CFL, dt, scale;
  // with VarMix%use_variable_mixing (:236-281)
  int use_VarMix, use_Eady, Resoln_scaled;
  double KhTr_Slope_Cff, KhTr_fac, KhTr_min, KhTr_max, pass_coeff, pass_min;
  const double *MEKE_Kh, *L2u, *L2v, *SN_u, *SN_v, *Res_fn_h, *Rd_dx_h;
  const double *h;
  double *khdt_x, *khdt_y;
  double *const *tr;       // device table of ntr tracer pointers
  double *const *work;     // device table of ntr work copies
  const double *cu;        // conc_underflow per tracer (device) or null
  unsigned long long *cfl_bits;
  int ntr, check_cfl;
  int nkml, nkmb;          // CS%Diffuse_ML_interior: GV%nkml, GV%nk_rho_varies (nkmb = 0: not in use)
  double ML_KhTr_scale;
};

// The diffusive flux diagnostics, handed to the DIAG instantiation of hd_step_kernel only (HDNoDiag otherwise: the instantiation without
// diagnostics is what it was): device tables of ntr pointers to face-shaped scratch (null: the tracer did not ask), which take
// Coef_x(I,j,1) * (t(i,j,k) - t(i+1,j,k)) * Idt of the iteration, and the y twin (:576-591); flux_diag_march_kernel adds them up.
struct HDDiag { double *const *sx, *const *sy; double Idt; };
struct HDNoDiag {};
template <bool DIAG> using HDDiagArg = std::conditional_t<DIAG, HDDiag, HDNoDiag>;

// the scale of layer k (0-based) :543-550; false: the layer is left out of the along-layer diffusion
__device__ __forceinline__ bool hd_layer_scale(const HDArgs &A, int k, double &scale) {
  scale = A.scale;
  if (A.nkmb > 0) {
    if (k + 1 <= A.nkml) {
      if (A.ML_KhTr_scale <= 0.0) return false;
      scale = A.scale * A.ML_KhTr_scale;
    }
    if ((k + 1 > A.nkml) && (k + 1 <= A.nkmb)) return false;
  }
  return true;
}

// the diffusivity of a face with variable mixing :236-281 (c0, c1: the cells either side; f: the face)
__device__ __forceinline__ double hd_Kh_face(const HDArgs &A, long c0, long c1, long f, bool dir) {
  double Kh_loc = A.KhTr;
  if (A.use_Eady) Kh_loc = Kh_loc + A.KhTr_Slope_Cff * (dir ? A.L2v[f] : A.L2u[f]) * (dir ? A.SN_v[f] : A.SN_u[f]);
  if (A.MEKE_Kh) Kh_loc = Kh_loc + A.KhTr_fac * sqrt(A.MEKE_Kh[c0] * A.MEKE_Kh[c1]);
  if (A.KhTr_max > 0.) Kh_loc = min2(Kh_loc, A.KhTr_max);
  if (A.Resoln_scaled) Kh_loc = Kh_loc * 0.5 * (A.Res_fn_h[c0] + A.Res_fn_h[c1]);
  double Kh = max2(Kh_loc, A.KhTr_min);
  if (A.pass_coeff > 0.) {
    const double Rd_dx = 0.5 * (A.Rd_dx_h[c0] + A.Rd_dx_h[c1]);
    Kh_loc = Kh * max2(A.pass_min, A.pass_coeff * Rd_dx);
    if (A.KhTr_max > 0.) Kh_loc = min2(Kh_loc, A.KhTr_max);
    Kh = max2(Kh_loc, A.KhTr_min);
  }
  return Kh;
}

// thread (i, j) over (is-1 : ie, js-1 : je)
__global__ __launch_bounds__(256) void hd_khdt_kernel(HDArgs A) {
  const m6::GridDev &g = A.g;
  const int i = g.isc - 1 + blockIdx.x * blockDim.x + threadIdx.x, j = g.jsc - 1 + blockIdx.y;
  if (i > g.iec) return;
  const int I = i, J = j;
  if (j >= g.jsc) {      // khdt_x(I,j), I = is-1 .. ie
    const double Kh = A.use_VarMix ? hd_Kh_face(A, g.h2(i, j), g.h2(i + 1, j), g.u2(I, j), false) : A.KhTr;
    double kx = A.dt * (Kh * (g.dy_Cu[g.u2(I, j)] * g.IdxCu[g.u2(I, j)]));
    if (A.max_diff_CFL > 0.0) kx = min2(kx, 0.125 * A.max_diff_CFL * min2(g.areaT[g.h2(i, j)], g.areaT[g.h2(i + 1, j)]));
    A.khdt_x[g.u2(I, j)] = kx;
  }
  if (i >= g.isc) {      // khdt_y(i,J), J = js-1 .. je
    const double Kh = A.use_VarMix ? hd_Kh_face(A, g.h2(i, j), g.h2(i, j + 1), g.v2(i, J), true) : A.KhTr;
    double ky = A.dt * (Kh * (g.dx_Cv[g.v2(i, J)] * g.IdyCv[g.v2(i, J)]));
    if (A.max_diff_CFL > 0.0) ky = min2(ky, 0.125 * A.max_diff_CFL * min2(g.areaT[g.h2(i, j)], g.areaT[g.h2(i, j + 1)]));
    A.khdt_y[g.v2(i, J)] = ky;
  }
}

// thread (i, j) over the compute domain: CFL(i,j) :412-414 and its maximum
__global__ __launch_bounds__(256) void hd_cfl_kernel(HDArgs A) {
  const m6::GridDev &g = A.g;
  const int i = g.isc + blockIdx.x * blockDim.x + threadIdx.x, j = g.jsc + blockIdx.y;
  double cfl = 0.0;
  if (i <= g.iec) {
    const int I = i, J = j;
    cfl = 2.0 * ((A.khdt_x[g.u2(I - 1, j)] + A.khdt_x[g.u2(I, j)]) + (A.khdt_y[g.v2(i, J - 1)] + A.khdt_y[g.v2(i, J)])) * g.IareaT[g.h2(i, j)];
  }
  unsigned long long b = (unsigned long long)__double_as_longlong(cfl > 0.0 ? cfl : 0.0);      // positive doubles order as integers
  for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_down(b, off); b = o > b ? o : b; }
  if ((threadIdx.x & 63) == 0) atomicMax(A.cfl_bits, b);
}

// thread (i, j, k) over the compute domain.  DIAG: the thread stores the values of its east and north face, and of the west and south
// face where it is the first cell of its row or column (I = IscB..IecB, j = js..je; J = JscB..JecB, i = is..ie).
template <bool DIAG = false>
__global__ __launch_bounds__(256) void hd_step_kernel(HDArgs A, HDDiagArg<DIAG> d) {
  const m6::GridDev &g = A.g;
  const int i = g.isc + blockIdx.x * blockDim.x + threadIdx.x, j = g.jsc + blockIdx.y, k = blockIdx.z;
  if (i > g.iec) return;
  const int I = i, J = j;
  const long kH = (long)g.nih * g.njh * k;
  const double *h = A.h + kH;
  const double h_neglect = g.H_subroundoff;
  double scale;
  if (!hd_layer_scale(A, k, scale)) return;
  const double hc = h[g.h2(i, j)], hw = h[g.h2(i - 1, j)], he = h[g.h2(i + 1, j)], hs = h[g.h2(i, j - 1)], hn = h[g.h2(i, j + 1)];
  // Coef_x(I-1,j), Coef_x(I,j), Coef_y(i,J-1), Coef_y(i,J) :552-561
  const double CxW = ((scale * A.khdt_x[g.u2(I - 1, j)]) * 2.0 * (hw * hc)) / (hw + hc + h_neglect);
  const double CxE = ((scale * A.khdt_x[g.u2(I, j)]) * 2.0 * (hc * he)) / (hc + he + h_neglect);
  const double CyS = ((scale * A.khdt_y[g.v2(i, J - 1)]) * 2.0 * (hs * hc)) / (hs + hc + h_neglect);
  const double CyN = ((scale * A.khdt_y[g.v2(i, J)]) * 2.0 * (hc * hn)) / (hc + hn + h_neglect);
  const double Ihdxdy = g.IareaT[g.h2(i, j)] / (hc + h_neglect);
  for (int m = 0; m < A.ntr; m++) {
    const double *t = A.tr[m] + kH;
    const double tc = t[g.h2(i, j)];
    const double dTr = Ihdxdy * ((CxW * (t[g.h2(i - 1, j)] - tc) - CxE * (tc - t[g.h2(i + 1, j)])) +
                                 (CyS * (t[g.h2(i, j - 1)] - tc) - CyN * (tc - t[g.h2(i, j + 1)])));
    A.work[m][kH + g.h2(i, j)] = tc + dTr;
    if constexpr (DIAG) {
      const long uH = (long)(g.nih + 1) * g.njh * k, vH = (long)g.nih * (g.njh + 1) * k;
      if (d.sx[m]) {
        d.sx[m][uH + g.u2(I, j)] = (CxE * (tc - t[g.h2(i + 1, j)])) * d.Idt;
        if (i == g.isc) d.sx[m][uH + g.u2(I - 1, j)] = (CxW * (t[g.h2(i - 1, j)] - tc)) * d.Idt;
      }
      if (d.sy[m]) {
        d.sy[m][vH + g.v2(i, J)] = (CyN * (tc - t[g.h2(i, j + 1)])) * d.Idt;
        if (j == g.jsc) d.sy[m][vH + g.v2(i, J - 1)] = (CyS * (t[g.h2(i, j - 1)] - tc)) * d.Idt;
      }
    }
  }
}

__global__ __launch_bounds__(256) void hd_commit_kernel(HDArgs A) {
  const m6::GridDev &g = A.g;
  const int i = g.isc + blockIdx.x * blockDim.x + threadIdx.x, j = g.jsc + blockIdx.y, k = blockIdx.z;
  if (i > g.iec) return;
  const long n = (long)g.nih * g.njh * k + g.h2(i, j);
  double scale;
  const bool stepped = hd_layer_scale(A, k, scale);      // a layer that was left out has no work copy: only the underflow applies
  for (int m = 0; m < A.ntr; m++) {
    double x = stepped ? A.work[m][n] : A.tr[m][n];
    if (A.cu && A.cu[m] > 0.0 && fabs(x) < A.cu[m]) x = 0.0;
    A.tr[m][n] = x;
  }
}

}  // namespace

// what an entry point hands on beside the arguments all of them have: the control structures it takes, and whether it is the one
// that takes DIFFUSE_ML_TO_INTERIOR (epi) or USE_HORIZONTAL_BOUNDARY_DIFFUSION (hbd)
struct HordiffOpts {
  const mom6hip_neutral_diffusion_cs_t *nd;
  const mom6hip_epipycnal_cs_t *epi;
  const mom6hip_hor_bnd_diffusion_cs_t *hbd;
  const mom6hip_ndiff_discontinuous_cs_t *ndd;
  const mom6hip_eos_t *eos;
  const double *p_surf;
  int32_t idx_T, idx_S;
  bool takes_epi, takes_hbd;
  const mom6hip_tracer_flux_diag_t *diag = nullptr;      // the diffusive flux diagnostics of the tracers (null: none)
  const mom6hip_tracer_mix_diag_t *mix = nullptr;        // what neutral_diffusion and hor_bnd_diffusion post themselves (null: none)
};

static int hordiff_impl(mom6hip_ctx_t *ctx, const mom6hip_tracer_hor_diff_cs_t *cs, const mom6hip_hordiff_fields_t *F, const double *h, double dt,
                        double *const *tr, const double *conc_underflow, int32_t ntr, int32_t memspace, mom6hip_hordiff_stats_t *stats,
                        const HordiffOpts &o) {
  M6_REQUIRE(cs != nullptr, "tracer_hordiff: null argument");
  // the branches an entry point does not take, and those that exclude each other (MOM_tracer_hor_diff.F90:1732, :1735)
  M6_REQUIRE(!(o.takes_epi && cs->unsupported[0]), "MOM_tracer_hor_diff: USE_NEUTRAL_DIFFUSION and DIFFUSE_ML_TO_INTERIOR are mutually exclusive!");
  M6_REQUIRE(!(o.takes_hbd && cs->unsupported[1] && cs->unsupported[2]),
             "MOM_tracer_hor_diff: USE_HORIZONTAL_BOUNDARY_DIFFUSION and DIFFUSE_ML_TO_INTERIOR are mutually exclusive!");
  M6_REQUIRE(o.takes_epi || !cs->unsupported[2], "tracer_hordiff: DIFFUSE_ML_TO_INTERIOR is not provided by this entry point (mom6hip_tracer_hordiff_epipycnal takes it)");
  M6_REQUIRE(!cs->unsupported[2] || o.epi != nullptr, "tracer_hordiff: DIFFUSE_ML_TO_INTERIOR needs its control structure (mom6hip_epipycnal_cs_t)");
  M6_REQUIRE(!(o.takes_hbd && cs->unsupported[1]) || o.hbd != nullptr, "tracer_hordiff: USE_HORIZONTAL_BOUNDARY_DIFFUSION needs its control structure (mom6hip_hor_bnd_diffusion_cs_t)");
  const mom6hip_neutral_diffusion_cs_t *nd = o.nd;
  const mom6hip_epipycnal_cs_t *epi = cs->unsupported[2] ? o.epi : nullptr;
  const mom6hip_hor_bnd_diffusion_cs_t *hbd = cs->unsupported[1] ? o.hbd : nullptr;
  static const char *names[8] = {"USE_NEUTRAL_DIFFUSION", "USE_HORIZONTAL_BOUNDARY_DIFFUSION", "DIFFUSE_ML_TO_INTERIOR",
                                 "(free)", "(free)", "KHTR_USE_EBT_STRUCT", "offline khdt (do_online = false)",
                                 "the df_x / df_y flux diagnostics"};
  M6_REQUIRE(ctx != nullptr, "MOM_tracer_hor_diff: register_tracer must be called before tracer_hordiff.");
  M6_REQUIRE(h != nullptr, "tracer_hordiff: null argument");
  M6_REQUIRE(memspace == MOM6HIP_MEM_HOST || memspace == MOM6HIP_MEM_DEVICE, "tracer_hordiff: bad memspace");
  // unsupported[5] (CS%KhTr_use_ebt_struct) is a switch every entry point takes: the neutral and the boundary-diffusion branch read
  // fields->ebt_struct, the along-layer and the epipycnal branch read level 1 of the coefficients only and ignore the field
  for (int q = 1; q < 8; q++)
    M6_REQUIRE(q == 2 || q == 5 || (q == 1 && hbd) || !cs->unsupported[q], "tracer_hordiff: %s is not provided by libmom6hip", names[q]);
  const bool use_neutral = cs->unsupported[0] != 0;      // CS%use_neutral_diffusion
  const bool use_hbd = hbd != nullptr;      // (the entry point takes it, and CS%use_hor_bnd_diffusion)
  const bool use_ebt = cs->unsupported[5] != 0 && (use_neutral || use_hbd);      // CS%KhTr_use_ebt_struct where ebt_struct is read
  M6_REQUIRE(!use_ebt || (F && F->ebt_struct), "tracer_hordiff: KHTR_USE_EBT_STRUCT needs VarMix%%ebt_struct (fields->ebt_struct)");
  M6_REQUIRE(!use_neutral || nd == nullptr || (nd->unsupported[3] != 0) == (cs->unsupported[5] != 0),
             "tracer_hordiff: KHTR_USE_EBT_STRUCT of the neutral_diffusion control structure (unsupported[3]) differs from that of "
             "tracer_hor_diff_CS (unsupported[5]); in the reference both are the one parameter");
  if (stats) { stats->num_itts = 0; stats->halo_updates = 0; stats->max_CFL = 0.0; }
  const bool use_VarMix = cs->use_variable_mixing != 0;
  if (ntr == 0 || (cs->KhTr <= 0.0 && !use_VarMix)) return 0;      // :197
  const bool use_Eady = use_VarMix && cs->KhTr_Slope_Cff > 0., Resoln_scaled = use_VarMix && cs->Resoln_scaled_KhTr;
  M6_REQUIRE(!use_Eady || (F && F->L2u && F->L2v && F->SN_u && F->SN_v), "tracer_hordiff: KHTR_SLOPE_CFF > 0 needs VarMix%%L2u, L2v, SN_u, SN_v");
  M6_REQUIRE(!Resoln_scaled || (F && F->Res_fn_h), "tracer_hordiff: RESOLN_SCALED_KHTR needs VarMix%%Res_fn_h");
  M6_REQUIRE(!(use_VarMix && cs->KhTr_passivity_coeff > 0.) || (F && F->Rd_dx_h), "tracer_hordiff: KHTR_PASSIVITY_COEFF > 0 needs VarMix%%Rd_dx_h");
  M6_REQUIRE(tr != nullptr && ntr > 0 && ntr <= 24, "tracer_hordiff: bad tracer list (at most 24 tracers)");
  M6_REQUIRE(dt > 0.0, "tracer_hordiff: dt must be positive");
  const m6::GridDev g = ctx->g;
  M6_REQUIRE(g.dy_Cu && g.IdxCu && g.dx_Cv && g.IdyCv && g.areaT && g.IareaT, "tracer_hordiff: dy_Cu, IdxCu, dx_Cv, IdyCv, areaT and IareaT are needed");
  M6_REQUIRE(g.isc - g.isd >= 1 && g.jsc - g.jsd >= 1, "tracer_hordiff: the halo must be at least 1 point wide");
  const size_t bH = sizeof(double) * (size_t)g.nh3();
  const size_t bU2 = sizeof(double) * (size_t)(g.nih + 1) * g.njh, bV2 = sizeof(double) * (size_t)g.nih * (g.njh + 1);
  hipStream_t s = ctx->stream;
  m6::Stager st(ctx, memspace);
  HDArgs A;
  A.g = g; A.KhTr = cs->KhTr; A.max_diff_CFL = cs->max_diff_CFL; A.dt = dt; A.ntr = ntr; A.check_cfl = cs->check_diffusive_CFL;
  A.h = st.in(h, bH);
  A.nkml = epi ? epi->nkml : 0; A.nkmb = epi ? epi->nk_rho_varies : 0; A.ML_KhTr_scale = epi ? epi->ML_KhTr_scale : 1.0;
  A.use_VarMix = use_VarMix; A.use_Eady = use_Eady; A.Resoln_scaled = Resoln_scaled;
  A.KhTr_Slope_Cff = cs->KhTr_Slope_Cff; A.KhTr_fac = cs->KhTr_fac; A.KhTr_min = cs->KhTr_min; A.KhTr_max = cs->KhTr_max;
  A.pass_coeff = use_VarMix ? cs->KhTr_passivity_coeff : 0.0; A.pass_min = cs->KhTr_passivity_min;
  {
    const size_t bH2 = sizeof(double) * (size_t)g.nih * g.njh;
    A.MEKE_Kh = (use_VarMix && F) ? st.in(F->MEKE_Kh, bH2) : nullptr;
    A.L2u = use_Eady ? st.in(F->L2u, bU2) : nullptr; A.L2v = use_Eady ? st.in(F->L2v, bV2) : nullptr;
    A.SN_u = use_Eady ? st.in(F->SN_u, bU2) : nullptr; A.SN_v = use_Eady ? st.in(F->SN_v, bV2) : nullptr;
    A.Res_fn_h = Resoln_scaled ? st.in(F->Res_fn_h, bH2) : nullptr;
    A.Rd_dx_h = (A.pass_coeff > 0.) ? st.in(F->Rd_dx_h, bH2) : nullptr;
  }
  std::vector<double *> d_tr(ntr), d_work(ntr);
  for (int m = 0; m < ntr; m++) {
    M6_REQUIRE(tr[m] != nullptr, "tracer_hordiff: tracer %d is null", m);
    d_tr[m] = st.inout(tr[m], bH);
    d_work[m] = use_neutral ? nullptr : (double *)st.scratch(bH);
  }
  // the diffusive flux diagnostics: device views of the arrays asked for (a host array is copied in and out: the call writes a range of
  // it, :389-406) and a face-shaped scratch each for the x and the y increments of a tracer that has any
  const size_t bU3 = bU2 * g.nk, bV3 = bV2 * g.nk;
  std::vector<std::array<double *, 4>> d_df(ntr, std::array<double *, 4>{});      // df_x, df_y, df2d_x, df2d_y
  std::vector<double *> d_sx(ntr, nullptr), d_sy(ntr, nullptr);
  bool any_df = false;
  if (o.diag) for (int m = 0; m < ntr; m++) {
    const mom6hip_tracer_flux_diag_t &D = o.diag[m];
    M6_REQUIRE(!(epi && (D.df2d_x || D.df2d_y)), "tracer_hordiff: df2d_x / df2d_y together with DIFFUSE_ML_TO_INTERIOR (the epipycnal "
               "contribution to the diffusive flux diagnostics) is not provided by libmom6hip");
    d_df[m] = {st.inout(D.df_x, bU3), st.inout(D.df_y, bV3), st.inout(D.df2d_x, bU2), st.inout(D.df2d_y, bV2)};
    any_df = any_df || D.df_x || D.df_y || D.df2d_x || D.df2d_y;
  }
  if (any_df && !use_neutral) {      // (one block: the pool of the context is short)
    size_t nx = 0, ny = 0;
    for (int m = 0; m < ntr; m++) { nx += (d_df[m][0] || d_df[m][2]) ? 1 : 0; ny += (d_df[m][1] || d_df[m][3]) ? 1 : 0; }
    char *q = (char *)st.scratch(nx * bU3 + ny * bV3);
    M6_REQUIRE(q != nullptr, "tracer_hordiff: out of device memory for the flux diagnostics");
    for (int m = 0; m < ntr; m++) {
      if (d_df[m][0] || d_df[m][2]) { d_sx[m] = (double *)q; q += bU3; }
      if (d_df[m][1] || d_df[m][3]) { d_sy[m] = (double *)q; q += bV3; }
    }
  }
  // the diagnostics of neutral_diffusion and hor_bnd_diffusion: device views of the arrays asked for.  Host arrays are staged through one
  // block (the pool of the context is short) once the iteration count has been accepted, copied in whole -- the call writes their compute
  // range only -- and copied back at the end
  static const char *mix_names[m6::MIX_COUNT] = {"dfx_2d", "dfy_2d", "dfxy_cont", "dfxy_cont_2d", "dfxy_conc", "hbd_dfx", "hbd_dfy", "hbd_dfx_2d",
                                                 "hbd_dfy_2d", "hbdxy_cont", "hbdxy_cont_2d", "hbdxy_conc"};
  const size_t mix_bytes[m6::MIX_COUNT] = {bU2, bV2, bH, bH / g.nk, bH, bU3, bV3, bU2, bV2, bH, bH / g.nk, bH};
  std::vector<m6::MixDiag> d_mix;
  struct MixBack { double *host, *dev; size_t bytes; };
  std::vector<MixBack> mix_back;
  bool any_mix = false;
  size_t mix_total = 0;
  if (o.mix) {
    d_mix.assign(ntr, m6::MixDiag{});
    size_t &total = mix_total;
    for (int m = 0; m < ntr; m++) {
      double *const p[m6::MIX_COUNT] = {o.mix[m].dfx_2d, o.mix[m].dfy_2d, o.mix[m].dfxy_cont, o.mix[m].dfxy_cont_2d, o.mix[m].dfxy_conc,
                                        o.mix[m].hbd_dfx, o.mix[m].hbd_dfy, o.mix[m].hbd_dfx_2d, o.mix[m].hbd_dfy_2d, o.mix[m].hbdxy_cont,
                                        o.mix[m].hbdxy_cont_2d, o.mix[m].hbdxy_conc};
      for (int q = 0; q < m6::MIX_COUNT; q++) {
        if (!p[q]) continue;
        any_mix = true;
        M6_REQUIRE(q >= m6::MIX_HBD_DFX || use_neutral, "tracer_hordiff: %s of tracer %d is a diagnostic of neutral_diffusion: it is refused "
                   "without USE_NEUTRAL_DIFFUSION", mix_names[q], m + 1);
        M6_REQUIRE(q < m6::MIX_HBD_DFX || use_hbd, "tracer_hordiff: %s of tracer %d is a diagnostic of hor_bnd_diffusion: it is refused "
                   "without USE_HORIZONTAL_BOUNDARY_DIFFUSION", mix_names[q], m + 1);
        d_mix[m].a[q] = p[q];
        if (memspace == MOM6HIP_MEM_HOST) { mix_back.push_back({p[q], nullptr, mix_bytes[q]}); total += mix_bytes[q]; }
      }
    }
  }
  A.khdt_x = (double *)st.scratch(bU2); A.khdt_y = (double *)st.scratch(bV2);
  char *tab = (char *)st.scratch(4 * 24 * sizeof(double *) + 24 * sizeof(double) + 16);
  M6_REQUIRE(!st.failed() && tab, "tracer_hordiff: staging failed");
  double **t_tr = (double **)tab, **t_work = t_tr + 24, **t_sx = t_work + 24, **t_sy = t_sx + 24;
  double *t_cu = (double *)(t_sy + 24);
  A.cfl_bits = (unsigned long long *)(t_cu + 24);
  M6_HIP(hipMemcpyAsync(t_tr, d_tr.data(), ntr * sizeof(double *), hipMemcpyHostToDevice, s));
  M6_HIP(hipMemcpyAsync(t_work, d_work.data(), ntr * sizeof(double *), hipMemcpyHostToDevice, s));
  M6_HIP(hipMemcpyAsync(t_sx, d_sx.data(), ntr * sizeof(double *), hipMemcpyHostToDevice, s));
  M6_HIP(hipMemcpyAsync(t_sy, d_sy.data(), ntr * sizeof(double *), hipMemcpyHostToDevice, s));
  std::vector<double> cu(ntr, 0.0);
  bool any_cu = false;
  if (conc_underflow) for (int m = 0; m < ntr; m++) { cu[m] = conc_underflow[m]; any_cu = any_cu || cu[m] > 0.0; }
  M6_HIP(hipMemcpyAsync(t_cu, cu.data(), ntr * sizeof(double), hipMemcpyHostToDevice, s));
  M6_HIP(hipMemsetAsync(A.cfl_bits, 0, sizeof(unsigned long long), s));
  M6_HIP(hipMemsetAsync(A.khdt_x, 0, bU2, s)); M6_HIP(hipMemsetAsync(A.khdt_y, 0, bV2, s));
  A.tr = t_tr; A.work = t_work; A.cu = any_cu ? t_cu : nullptr;
  M6_HIP(hipStreamSynchronize(s));      // the tables above live on the host stack

  const int ni = g.iec - g.isc + 1, nj = g.jec - g.jsc + 1;
  A.scale = 1.0;
  hipLaunchKernelGGL(hd_khdt_kernel, dim3((ni + 1 + 255) / 256, nj + 1), dim3(256), 0, s, A);
  int num_itts = 1;
  double max_CFL = 0.0;
  if (cs->check_diffusive_CFL) {      // :410-423
    hipLaunchKernelGGL(hd_cfl_kernel, dim3((ni + 255) / 256, nj), dim3(256), 0, s, A);
    unsigned long long bits = 0;
    M6_HIP(hipMemcpyAsync(&bits, A.cfl_bits, sizeof(bits), hipMemcpyDeviceToHost, s));
    M6_HIP(hipStreamSynchronize(s));
    memcpy(&max_CFL, &bits, 8);
    double neg = -max_CFL;      // max_across_PEs
    if (m6::multi_tile(ctx)) { if (int rc = m6::min_across_PEs(ctx, &neg, 1)) return rc; }
    max_CFL = -neg;
    num_itts = (int)ceil(max_CFL - 4.0 * DBL_EPSILON);
    if (num_itts < 1) num_itts = 1;
  } else if (cs->max_diff_CFL > 0.0) {
    num_itts = (int)ceil(cs->max_diff_CFL - 4.0 * DBL_EPSILON);
    if (num_itts < 1) num_itts = 1;
  }
  A.scale = 1.0 / ((double)num_itts);      // I_numitts
  M6_HIP(hipGetLastError());
  // neutral_diffusion and hor_bnd_diffusion post once an iteration of the itt loop, and the posts are separate
  M6_REQUIRE(!(any_mix && num_itts > 1), "tracer_hordiff: the diagnostics of neutral_diffusion and hor_bnd_diffusion (dfx_2d .. dfxy_conc, "
             "hbd_*) are posted once an iteration by the reference: with num_itts = %d iterations (MAX_TR_DIFFUSION_CFL, CHECK_DIFFUSIVE_CFL) "
             "they are not provided by libmom6hip", num_itts);
  if (mix_total) {      // (staged only after the refusal above: a call that is refused copies nothing)
    char *q = (char *)st.scratch(mix_total);
    M6_REQUIRE(!st.failed() && q, "tracer_hordiff: out of device memory for the diagnostics");
    size_t at = 0;
    for (int m = 0; m < ntr; m++) for (int w = 0; w < m6::MIX_COUNT; w++) if (d_mix[m].a[w]) {
      MixBack &e = mix_back[at++];
      e.dev = (double *)q; q += e.bytes; d_mix[m].a[w] = e.dev;
      M6_HIP(hipMemcpyAsync(e.dev, e.host, e.bytes, hipMemcpyHostToDevice, s));
    }
  }

  std::vector<double *> pf(d_tr);
  std::vector<int32_t> ppos(ntr, MOM6HIP_POS_H), pnk(ntr, g.nk);
  int halo_updates = 0;
  const double *d_ebt = use_ebt ? st.in(F->ebt_struct, bH) : nullptr;
  // visc%h_ML where a branch reads it: the boundary diffusion, and the neutral branch with NDIFF_INTERIOR_ONLY
  const bool reads_h_ML = F && F->h_ML && (use_hbd || (use_neutral && nd && nd->interior_only));
  const double *d_hml = reads_h_ML ? st.in(F->h_ML, sizeof(double) * (size_t)g.nih * g.njh) : nullptr;
  const double *d_ps = (use_neutral && o.p_surf) ? st.in(o.p_surf, sizeof(double) * (size_t)g.nih * g.njh) : nullptr;
  M6_REQUIRE(!st.failed(), "tracer_hordiff: staging failed");
  const m6::HordiffCall call = {ctx, st, A.h, A.khdt_x, A.khdt_y, num_itts, A.scale, d_tr, cu, o.idx_T, o.idx_S, o.eos, d_ps, d_hml, d_ebt, &halo_updates,
                                  any_mix ? d_mix.data() : nullptr, 1.0 / (A.scale * dt)};
  // the march over k of the diagnostics asked for, in direction dir: zero = 1 sets them to zero over their ranges (:389-406), zero = 0 adds
  // what hd_step_kernel has just left in the scratch, but for the layers the along-layer loop leaves out (:544-550)
  auto df_march = [&](int dir, int zero) {
    m6::FluxDiagMarch a; a.g = g; a.doi = nullptr; a.zero = zero; a.is = g.isc; a.ie = g.iec; a.js = g.jsc; a.je = g.jec; a.n = 0;
    a.skip0 = a.skip1 = 0;
    if (A.nkmb > 0) { a.skip0 = (A.ML_KhTr_scale <= 0.0) ? 0 : A.nkml; a.skip1 = A.nkmb > a.skip0 ? A.nkmb : a.skip0; }
    for (int m = 0; m < ntr; m++) {
      if (!(d_df[m][dir] || d_df[m][2 + dir])) continue;
      a.face[a.n] = dir ? d_sy[m] : d_sx[m]; a.a3[a.n] = d_df[m][dir]; a.a2[a.n] = d_df[m][2 + dir];
      if (++a.n == m6::FLUX_DIAG_MAXD) { m6::flux_diag_march(dir, a, s); a.n = 0; }
    }
    if (a.n) m6::flux_diag_march(dir, a, s);
  };
  if (any_df) { df_march(0, 1); df_march(1, 1); }
  const HDDiag hd_diag = {t_sx, t_sy, 1.0 / dt};      // Idt :204
  if (use_hbd) {      // :408-472, before the neutral or the along-layer branch
    if (int rc = m6::hbd_branch(call, hbd, cs->KhTr_min, cs->full_depth_khtr_min != 0)) return rc;
  }
  if (use_neutral) {      // :474-534
    if (int rc = m6::neutral_branch(call, nd, o.ndd)) return rc;
  } else
  for (int itt = 1; itt <= num_itts; itt++) {      // :540-614
    if (int rc = m6::group_pass(ctx, pf.data(), ppos.data(), pnk.data(), ntr)) return rc;
    halo_updates++;
    if (any_df) {
      hipLaunchKernelGGL(hd_step_kernel<true>, dim3((ni + 255) / 256, nj, g.nk), dim3(256), 0, s, A, hd_diag);
      df_march(0, 0); df_march(1, 0);
    } else
      hipLaunchKernelGGL(hd_step_kernel<false>, dim3((ni + 255) / 256, nj, g.nk), dim3(256), 0, s, A, HDNoDiag{});
    hipLaunchKernelGGL(hd_commit_kernel, dim3((ni + 255) / 256, nj, g.nk), dim3(256), 0, s, A);
  }
  M6_HIP(hipGetLastError());
  if (epi) {      // :613-620
    if (int rc = m6::epipycnal_branch(call, epi)) return rc;
  }
  if (stats) { stats->num_itts = num_itts; stats->halo_updates = halo_updates; stats->max_CFL = max_CFL; }
  for (const MixBack &e : mix_back) M6_HIP(hipMemcpyAsync(e.host, e.dev, e.bytes, hipMemcpyDeviceToHost, s));      // (finish synchronises)
  return st.finish();
}


extern "C" int mom6hip_tracer_hordiff(mom6hip_ctx_t *ctx, const mom6hip_tracer_hor_diff_cs_t *cs, const double *h, double dt,
                                      double *const *tr, const double *conc_underflow, int32_t ntr, int32_t memspace,
                                      mom6hip_hordiff_stats_t *stats) {
  return mom6hip_tracer_hordiff_varmix(ctx, cs, nullptr, h, dt, tr, conc_underflow, ntr, memspace, stats);
}

extern "C" int mom6hip_tracer_hordiff_varmix(mom6hip_ctx_t *ctx, const mom6hip_tracer_hor_diff_cs_t *cs, const mom6hip_hordiff_fields_t *F,
                                             const double *h, double dt, double *const *tr, const double *conc_underflow, int32_t ntr,
                                             int32_t memspace, mom6hip_hordiff_stats_t *stats) {
  M6_REQUIRE(cs != nullptr, "tracer_hordiff: null argument");
  M6_REQUIRE(!cs->unsupported[0], "tracer_hordiff: USE_NEUTRAL_DIFFUSION is not provided by this entry point (mom6hip_tracer_hordiff_neutral takes it)");
  return mom6hip_tracer_hordiff_neutral(ctx, cs, nullptr, F, h, nullptr, nullptr, dt, tr, conc_underflow, ntr, 0, 0, memspace, stats);
}

extern "C" int mom6hip_tracer_hordiff_diag(mom6hip_ctx_t *ctx, const mom6hip_tracer_hor_diff_cs_t *cs, const mom6hip_hordiff_fields_t *F,
                                           const double *h, double dt, double *const *tr, const double *conc_underflow, int32_t ntr,
                                           int32_t memspace, mom6hip_hordiff_stats_t *stats, const mom6hip_tracer_flux_diag_t *diag) {
  M6_REQUIRE(cs != nullptr, "tracer_hordiff: null argument");
  M6_REQUIRE(!cs->unsupported[0], "tracer_hordiff: USE_NEUTRAL_DIFFUSION is not provided by this entry point (mom6hip_tracer_hordiff_neutral takes it)");
  HordiffOpts o = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, false, false};
  o.diag = diag;
  return hordiff_impl(ctx, cs, F, h, dt, tr, conc_underflow, ntr, memspace, stats, o);
}

extern "C" int mom6hip_tracer_hordiff_neutral(mom6hip_ctx_t *ctx, const mom6hip_tracer_hor_diff_cs_t *cs, const mom6hip_neutral_diffusion_cs_t *nd,
                                              const mom6hip_hordiff_fields_t *F, const double *h, const mom6hip_eos_t *eos, const double *p_surf,
                                              double dt, double *const *tr, const double *conc_underflow, int32_t ntr, int32_t idx_T,
                                              int32_t idx_S, int32_t memspace, mom6hip_hordiff_stats_t *stats) {
  const HordiffOpts o = {nd, nullptr, nullptr, nullptr, eos, p_surf, idx_T, idx_S, false, false};
  return hordiff_impl(ctx, cs, F, h, dt, tr, conc_underflow, ntr, memspace, stats, o);
}

extern "C" int mom6hip_tracer_hordiff_epipycnal(mom6hip_ctx_t *ctx, const mom6hip_tracer_hor_diff_cs_t *cs, const mom6hip_epipycnal_cs_t *epi,
                                                const mom6hip_hordiff_fields_t *F, const double *h, const mom6hip_eos_t *eos, double dt,
                                                double *const *tr, const double *conc_underflow, int32_t ntr, int32_t idx_T, int32_t idx_S,
                                                int32_t memspace, mom6hip_hordiff_stats_t *stats) {
  const HordiffOpts o = {nullptr, epi, nullptr, nullptr, eos, nullptr, idx_T, idx_S, true, false};
  return hordiff_impl(ctx, cs, F, h, dt, tr, conc_underflow, ntr, memspace, stats, o);
}

// DIFFUSE_ML_TO_INTERIOR with df_x / df_y: the layers :544-550 leave out stay zero; df2d_x / df2d_y would need the epipycnal contribution
// (:1405, :1526) and are refused by name in hordiff_impl
extern "C" int mom6hip_tracer_hordiff_epipycnal_diag(mom6hip_ctx_t *ctx, const mom6hip_tracer_hor_diff_cs_t *cs, const mom6hip_epipycnal_cs_t *epi,
                                                     const mom6hip_hordiff_fields_t *F, const double *h, const mom6hip_eos_t *eos, double dt,
                                                     double *const *tr, const double *conc_underflow, int32_t ntr, int32_t idx_T, int32_t idx_S,
                                                     int32_t memspace, mom6hip_hordiff_stats_t *stats, const mom6hip_tracer_flux_diag_t *diag) {
  HordiffOpts o = {nullptr, epi, nullptr, nullptr, eos, nullptr, idx_T, idx_S, true, false};
  o.diag = diag;
  return hordiff_impl(ctx, cs, F, h, dt, tr, conc_underflow, ntr, memspace, stats, o);
}

extern "C" int mom6hip_tracer_hordiff_hbd(mom6hip_ctx_t *ctx, const mom6hip_tracer_hor_diff_cs_t *cs, const mom6hip_hor_bnd_diffusion_cs_t *hbd,
                                          const mom6hip_neutral_diffusion_cs_t *nd, const mom6hip_hordiff_fields_t *F, const double *h,
                                          const mom6hip_eos_t *eos, const double *p_surf, double dt, double *const *tr,
                                          const double *conc_underflow, int32_t ntr, int32_t idx_T, int32_t idx_S, int32_t memspace,
                                          mom6hip_hordiff_stats_t *stats) {
  const HordiffOpts o = {nd, nullptr, hbd, nullptr, eos, p_surf, idx_T, idx_S, false, true};
  return hordiff_impl(ctx, cs, F, h, dt, tr, conc_underflow, ntr, memspace, stats, o);
}

// the same with the parameters of NDIFF_CONTINUOUS = False; hbd is read with USE_HORIZONTAL_BOUNDARY_DIFFUSION only
extern "C" int mom6hip_tracer_hordiff_neutral_discontinuous(mom6hip_ctx_t *ctx, const mom6hip_tracer_hor_diff_cs_t *cs,
                                                            const mom6hip_hor_bnd_diffusion_cs_t *hbd, const mom6hip_neutral_diffusion_cs_t *nd,
                                                            const mom6hip_ndiff_discontinuous_cs_t *ndd, const mom6hip_hordiff_fields_t *F,
                                                            const double *h, const mom6hip_eos_t *eos, const double *p_surf, double dt,
                                                            double *const *tr, const double *conc_underflow, int32_t ntr, int32_t idx_T,
                                                            int32_t idx_S, int32_t memspace, mom6hip_hordiff_stats_t *stats) {
  const HordiffOpts o = {nd, nullptr, hbd, ndd, eos, p_surf, idx_T, idx_S, false, true};
  return hordiff_impl(ctx, cs, F, h, dt, tr, conc_underflow, ntr, memspace, stats, o);
}

// the same with the diagnostics neutral_diffusion and hor_bnd_diffusion post themselves; diag == NULL: the call above
extern "C" int mom6hip_tracer_hordiff_mix_diag(mom6hip_ctx_t *ctx, const mom6hip_tracer_hor_diff_cs_t *cs, const mom6hip_hor_bnd_diffusion_cs_t *hbd,
                                               const mom6hip_neutral_diffusion_cs_t *nd, const mom6hip_ndiff_discontinuous_cs_t *ndd,
                                               const mom6hip_hordiff_fields_t *F, const double *h, const mom6hip_eos_t *eos, const double *p_surf,
                                               double dt, double *const *tr, const double *conc_underflow, int32_t ntr, int32_t idx_T,
                                               int32_t idx_S, int32_t memspace, mom6hip_hordiff_stats_t *stats,
                                               const mom6hip_tracer_mix_diag_t *diag) {
  HordiffOpts o = {nd, nullptr, hbd, ndd, eos, p_surf, idx_T, idx_S, false, true};
  o.mix = diag;
  return hordiff_impl(ctx, cs, F, h, dt, tr, conc_underflow, ntr, memspace, stats, o);
}

extern "C" uint64_t mom6hip_abi_sizeof_tracer_mix_diag(void) { return sizeof(mom6hip_tracer_mix_diag_t); }
extern "C" uint64_t mom6hip_abi_sizeof_tracer_hor_diff_cs(void) { return sizeof(mom6hip_tracer_hor_diff_cs_t); }
extern "C" uint64_t mom6hip_abi_sizeof_epipycnal_cs(void) { return sizeof(mom6hip_epipycnal_cs_t); }
extern "C" uint64_t mom6hip_abi_sizeof_hordiff_stats(void) { return sizeof(mom6hip_hordiff_stats_t); }
