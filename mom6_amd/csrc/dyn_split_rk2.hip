// dyn_split_rk2.hip -- step_MOM_dyn_split_RK2 on MI355X: the orchestration of the split RK2 step and its own
// streaming sweeps (src/core/MOM_dynamics_split_RK2.F90:289-1176; state initialisation :1521-1622).
//
// The whole step is enqueued on the context's stream in the reference's order: PressureForce, [CorAdCalc],
// continuity[BT_cont], btcalc, bt_mass_source, btstep (predictor), continuity (predictor), CorAdCalc, btstep
// (corrector), continuity (corrector), [CorAdCalc for the next predictor], with the group passes of the reference at
// the reference's seams.  The momentum sweeps (:557-564, :582-589, :667-676, :785-787, :879-886, :930-939,
// :1000-1002, :1038-1053) are plain i-contiguous streaming kernels; each is HBM-bound at 24-40 B/cell.
// All arrays are device arrays: nothing is staged, and without hooks / multi-tile passes / calc_dtbt nothing
// synchronises with the host.
#include "common.hpp"

#include <cstdlib>
#include <initializer_list>
#include <utility>

namespace {

template <class F> __global__ void __launch_bounds__(256) range3d_kernel(int i0, int i1, int j0, int j1, F f) {
  const int i = i0 + blockIdx.x * 64 + threadIdx.x, j = j0 + blockIdx.y * 4 + threadIdx.y;
  if (i <= i1 && j <= j1) f(i, j, (int)blockIdx.z);
}
// one thread per (i, j, k) of an inclusive horizontal range, all layers, i fastest
template <class F> void launch3d(hipStream_t st, int i0, int i1, int j0, int j1, int nk, F f) {
  if (i1 < i0 || j1 < j0) return;
  dim3 grid((i1 - i0 + 64) / 64, (j1 - j0 + 4) / 4, nk), block(64, 4);
  hipLaunchKernelGGL(range3d_kernel<F>, grid, block, 0, st, i0, i1, j0, j1, f);
}

struct Sz { size_t h2, h3, u3, v3; };
Sz sizes(const m6::GridDev &g) {
  Sz s;
  s.h2 = sizeof(double) * (size_t)g.nih * g.njh; s.h3 = s.h2 * g.nk;
  s.u3 = sizeof(double) * (size_t)(g.nih + 1) * g.njh * g.nk; s.v3 = sizeof(double) * (size_t)g.nih * (g.njh + 1) * g.nk;
  return s;
}

// the fields of a group pass as the domain layer takes them: (array, position | P2D for one level | MOM6HIP_PASS_SCALAR_PAIR)
struct PassFields {
  std::vector<double *> f; std::vector<int32_t> pos, nk;
  PassFields(std::initializer_list<std::pair<double *, int>> fl, int nk3) {
    for (auto &e : fl) { f.push_back(e.first); pos.push_back(e.second & (3 | MOM6HIP_PASS_SCALAR_PAIR)); nk.push_back((e.second & 4) ? 1 : nk3); }
  }
};
int pass(mom6hip_ctx_t *ctx, std::initializer_list<std::pair<double *, int>> fl, int nk3) {
  PassFields p(fl, nk3);
  return m6::group_pass(ctx, p.f.data(), p.pos.data(), p.nk.data(), (int)p.f.size());
}
// The non-blocking form (start_group_pass / complete_group_pass, MOM_domain_infra.F90:1141-1182): the exchange runs on the
// communication stream while the compute stream goes on with whatever does not read the halos in flight.
int pass_start(mom6hip_ctx_t *ctx, std::initializer_list<std::pair<double *, int>> fl, int nk3, int seam = 0) {
  PassFields p(fl, nk3);
  if (int rc = m6::start_group_pass(ctx, p.f.data(), p.pos.data(), p.nk.data(), (int)p.f.size())) return rc;
  // MOM6HIP_BLOCKING_PASSES=1: every pass completes where it starts (G%nonblocking_updates = False; comparison runs)
  // (=N > 1: a bit mask of the seams of the step, in order, that complete at once -- debugging)
  static const int blocking = [] { const char *e = getenv("MOM6HIP_BLOCKING_PASSES"); return e ? atoi(e) : 0; }();
  const bool now = blocking == 1 || (blocking > 1 && ((blocking >> 1) >> seam) & 1);
  return now ? m6::complete_group_pass(ctx) : 0;
}
// MOM6HIP_VV_KVML_ONCE=0 (read once): every vertvisc call of a step forms the KV_ML_INVZ2 profile itself (comparison runs, bisecting)
bool kvml_once() {
  static const bool on = !(getenv("MOM6HIP_VV_KVML_ONCE") && atoi(getenv("MOM6HIP_VV_KVML_ONCE")) == 0);
  return on;
}
// Whether the rows of the tile are worth splitting around a pass in flight: the pass must leave the x halos final at its start
// (the tile spans x) and the tile must be tall enough to have inner rows.
bool split_rows(mom6hip_ctx_t *ctx) {
  const int W = ctx->host.isc - ctx->host.isd, nj = ctx->host.jec - ctx->host.jsc + 1;
  return m6::pass_leaves_x_final(ctx) && nj >= 4 * W + 8 && (m6::multi_tile(ctx) || ctx->poison_passes || ctx->split_rows_always);
}
// `work` (kernels that are pure functions of their inputs row by row, taking their rows from ctx->g) around the completion of the
// pass in flight: the rows at least a halo width inside the tile before it, the two bands along the edges after it.
template <class F> int around_pass(mom6hip_ctx_t *ctx, F work) {
  if (!split_rows(ctx)) {
    ctx->overlap[2]++;
    if (int rc = m6::complete_group_pass(ctx)) return rc;
    return work();
  }
  ctx->overlap[0]++;
  const int js = ctx->host.jsc, je = ctx->host.jec, W = ctx->host.isc - ctx->host.isd;
  m6::row_window(ctx, js + W, je - W);
  int rc = work();
  m6::row_window_reset(ctx);
  // (an error between start and complete: the exchange in flight is completed all the same, so that the context is left without
  // a pending pass and the FIRST error is the one reported, not "a pass is already in flight" from the next call)
  if (rc) { m6::ErrorKeeper keep; m6::complete_group_pass(ctx); return rc; }
  if ((rc = m6::complete_group_pass(ctx))) return rc;
  m6::row_window(ctx, js, js + W - 1);
  rc = work();
  if (!rc) { m6::row_window(ctx, je - W + 1, je); rc = work(); }
  m6::row_window_reset(ctx);
  return rc;
}
// The continuity around the completion of the pass in flight: its zonal pass reads a row at a time, so the tile's own rows go
// first, with the meridional faces and cells whose stencil stays inside them (mom6hip_continuity, ctx->cont_phase = 1); the halo
// rows and the two edges follow the completion (cont_phase = 2).  x first, no fold on this tile, rows worth splitting; otherwise
// the pass completes and the continuity is the one call it always was.
template <class F> int continuity_around_pass(mom6hip_ctx_t *ctx, F call) {
  const bool phased = split_rows(ctx) && (ctx->host.first_direction % 2) == 0 && !ctx->host.tripolar_n;
  if (!phased) {
    ctx->overlap[2]++;
    if (int rc = m6::complete_group_pass(ctx)) return rc;
    return call();
  }
  ctx->overlap[1]++;
  ctx->cont_phase = 1;
  int rc = call();
  ctx->cont_phase = 0;
  if (rc) { m6::ErrorKeeper keep; m6::complete_group_pass(ctx); return rc; }
  if ((rc = m6::complete_group_pass(ctx))) return rc;
  ctx->cont_phase = 2;
  rc = call();
  ctx->cont_phase = 0;
  return rc;
}
constexpr int PH = MOM6HIP_POS_H, PU = MOM6HIP_POS_U, PV = MOM6HIP_POS_V, P2D = 4;
constexpr int PUs = PU | MOM6HIP_PASS_SCALAR_PAIR, PVs = PV | MOM6HIP_PASS_SCALAR_PAIR;      // To_All+SCALAR_PAIR (:462)

int check(const mom6hip_dyn_split_rk2_cs_t *cs, const char *who) {
  M6_REQUIRE(cs != nullptr, "%s: null control structure", who);
  M6_REQUIRE(cs->begw == 0.0, "%s: BEGW /= 0 is not provided", who);
  M6_REQUIRE(!cs->split_bottom_stress, "%s: SPLIT_BOTTOM_STRESS is not provided", who);
  // (eqn_of_state may be null: no equation of state, the layered PressureForce branch with GV%Rlay / GV%g_prime)
  M6_REQUIRE(cs->continuity_CSp && cs->CoriolisAdv && cs->PressureForce_CSp && cs->barotropic_CSp,
             "%s: a sub-module control structure is missing", who);
  M6_REQUIRE(cs->CAu && cs->CAv && cs->CAu_pred && cs->CAv_pred && cs->PFu && cs->PFv && cs->diffu && cs->diffv && cs->visc_rem_u &&
                 cs->visc_rem_v && cs->u_accel_bt && cs->v_accel_bt && cs->u_av && cs->v_av && cs->h_av && cs->pbce && cs->eta &&
                 cs->eta_PF && cs->uhbt && cs->vhbt, "%s: an array of the control structure is not allocated", who);
  return 0;
}

#define CALL(x) do { if (int rc_ = (x)) return rc_; } while (0)

// The surface pressure of a step (MOM_dynamics_split_RK2.F90:435-442): p_surf_end when both p_surf_begin and p_surf_end are given
// (dyn_p_surf), else forces%p_surf; and, after PressureForce, the eta that corresponds to the starting pressure (:497-503), which
// btstep takes as eta_PF_start (null without dyn_p_surf).
const double *step_p_surf(const mom6hip_dyn_split_rk2_cs_t *cs) {
  return (cs->p_surf_begin && cs->p_surf_end) ? cs->p_surf_end : cs->p_surf;
}
int step_eta_PF_start(mom6hip_ctx_t *ctx, const mom6hip_dyn_split_rk2_cs_t *cs, double **out) {
  *out = nullptr;
  if (!(cs->p_surf_begin && cs->p_surf_end)) return 0;
  const m6::GridDev g = ctx->g;
  const size_t bytes = (size_t)g.nih * g.njh * sizeof(double);
  M6_REQUIRE(ctx->rk2_eta_PF_start.reserve(bytes) == 0 && ctx->rk2_eta_PF_start.p, "step_MOM_dyn_split_RK2: out of device memory");
  double *eps = (double *)ctx->rk2_eta_PF_start.p;
  M6_HIP(hipMemsetAsync(eps, 0, bytes, ctx->stream));                                                // :439
  const double pres_to_eta = 1.0 / (g.g_Earth * (g.Rho0 * g.H_to_Z));                                // 1 / (GV%g_Earth * GV%H_to_RZ), Boussinesq
  const double *eta_PF = cs->eta_PF, *pb = cs->p_surf_begin, *pe = cs->p_surf_end;
  launch3d(ctx->stream, g.isc - 1, g.iec + 1, g.jsc - 1, g.jec + 1, 1, [=] __device__(int i, int j, int) {      // Isq .. Ieq+1, Jsq .. Jeq+1
    const long n = g.h2(i, j);
    eps[n] = eta_PF[n] - pres_to_eta * (pb[n] - pe[n]);
  });
  *out = eps;
  return 0;
}

// ---- the state of one call of a stepper ---------------------------------------------------------------------------------------
// Value-initialised in the entry, filled by step_call and step_scratch.  The velocities go by their role in the step: u_inst, v_inst
// are the instantaneous and u_av, v_av the filtered ones, whichever of the two pairs is the caller's argument (RK2: u_inst; RK2B:
// u_av) and whichever lives in the control structure (cs->u_av).
struct StepCall {
  mom6hip_ctx_t *ctx; mom6hip_dyn_split_rk2_cs_t *cs; m6::GridDev g; Sz sz; hipStream_t s;
  int is, ie, js, je, Isq, Ieq, Jsq, Jeq, nz;
  mom6hip_barotropic_cs_t *BT; const mom6hip_bt_cont_t *BTC; bool BT_cont_BT_thick;
  mom6hip_vertvisc_cs_t *VV; const mom6hip_visc_hooks_t *hk; const mom6hip_obc_t *OBC;
  double *u_inst, *v_inst, *u_av, *v_av, *h; const double *T, *Sal, *taux, *tauy;      // tv%T, tv%S, forces%taux, %tauy
  double *uh, *vh, *uhtr, *vhtr, *eta_av;
  double dt, dt_pred, RZ_to_H; int32_t calc_dtbt;
  double *up, *u_bc, *uh_in, *vp, *v_bc, *vh_in, *hp, *eta_pred, *u_old, *v_old;      // the step's automatic arrays (:336-369), step_scratch
  double *eta_PF_start;
  const char *who;      // the reference's name of the routine, for the messages
};
void step_call(StepCall &S, mom6hip_ctx_t *ctx, mom6hip_dyn_split_rk2_cs_t *cs, const char *who, double *u_inst, double *v_inst, double *u_av,
               double *v_av, double *h, const double *T, const double *Sal, double dt, const double *taux, const double *tauy, double RZ_to_H,
               double *uh, double *vh, double *uhtr, double *vhtr, double *eta_av, int32_t calc_dtbt) {
  S.ctx = ctx; S.cs = cs; S.g = ctx->g; S.sz = sizes(S.g); S.s = ctx->stream; S.who = who;
  S.is = S.g.isc; S.ie = S.g.iec; S.js = S.g.jsc; S.je = S.g.jec; S.nz = S.g.nk;
  S.Isq = S.is - 1; S.Ieq = S.ie; S.Jsq = S.js - 1; S.Jeq = S.je;
  S.BT = cs->barotropic_CSp; S.BTC = cs->BT_cont; S.BT_cont_BT_thick = S.BTC && S.BTC->h_u && S.BTC->h_v;
  S.VV = cs->vertvisc_CSp; S.hk = cs->hooks; S.OBC = cs->OBC;
  S.u_inst = u_inst; S.v_inst = v_inst; S.u_av = u_av; S.v_av = v_av; S.h = h; S.T = T; S.Sal = Sal; S.taux = taux; S.tauy = tauy;
  S.uh = uh; S.vh = vh; S.uhtr = uhtr; S.vhtr = vhtr; S.eta_av = eta_av;
  S.dt = dt; S.dt_pred = dt * cs->be; S.RZ_to_H = RZ_to_H; S.calc_dtbt = calc_dtbt;
}

// The step's automatic arrays (:336-369): one grow-only block in the context's pool (its own buffer: the modules the step calls hand out
// the pool's buffers from the start in every call), up u_bc uh_in | vp v_bc vh_in | hp | eta_pred, and behind them u_old_rad_OBC,
// v_old_rad_OBC (:360-363) when an OBC is associated.
// up = vp = 0 (:419-421).  The zeros only matter where nothing writes afterwards: the halo faces beyond a closed edge (every other point of
// up, vp is recomputed or refilled by pass_uvp each step; u_bc_accel, uh_in and eta_pred are read only where they are written), so the
// block is zeroed when it grows, not every step -- and when another stepper used it last (`tag`): the steppers leave different values
// at those faces.
int step_scratch(StepCall &S, int tag) {
  mom6hip_ctx_t *ctx = S.ctx;
  const Sz &sz = S.sz;
  const size_t blk_bytes = 3 * sz.u3 + 3 * sz.v3 + sz.h3 + sz.h2 + (S.OBC ? sz.u3 + sz.v3 : 0);
  const bool fresh = ctx->rk2_scratch.bytes < blk_bytes || ctx->rk2_scratch_layout != tag;
  M6_REQUIRE(ctx->rk2_scratch.reserve(blk_bytes) == 0, "%s: out of device memory", S.who);
  ctx->rk2_scratch_layout = tag;
  char *blk = (char *)ctx->rk2_scratch.p;
  S.up = (double *)blk; S.u_bc = (double *)(blk + sz.u3); S.uh_in = (double *)(blk + 2 * sz.u3);
  S.vp = (double *)(blk + 3 * sz.u3); S.v_bc = (double *)(blk + 3 * sz.u3 + sz.v3); S.vh_in = (double *)(blk + 3 * sz.u3 + 2 * sz.v3);
  S.hp = (double *)(blk + 3 * sz.u3 + 3 * sz.v3); S.eta_pred = (double *)(blk + 3 * sz.u3 + 3 * sz.v3 + sz.h3);
  if (S.OBC) { S.u_old = (double *)(blk + 3 * sz.u3 + 3 * sz.v3 + sz.h3 + sz.h2); S.v_old = (double *)((char *)S.u_old + sz.u3); }
  if (fresh) M6_HIP(hipMemsetAsync(blk, 0, blk_bytes, S.s));
  return 0;
}

// ---- the step's own sweeps, each written once: plain i-contiguous streaming kernels over the pointers and scalars they read ---------

// u_bc_accel = (CAu + PFu) + diffu (:557-564, :879-886) and, with u0, v0, the first up = mask*(u0 + dt*u_bc_accel) (:582-589) in the
// same sweep.  inviscid: diffu = diffv = +0.0 everywhere (set by dyn_split_rk2_init): (a + 0.0) is a, except that -0.0 + 0.0 = +0.0, so
// the array need not be read.
void bc_accel(const StepCall &S, const double *CAu, const double *CAv, bool inviscid, const double *u0, const double *v0) {
  const m6::GridDev g = S.g;
  const double *PFu = S.cs->PFu, *PFv = S.cs->PFv, *diffu = S.cs->diffu, *diffv = S.cs->diffv;
  double *u_bc = S.u_bc, *v_bc = S.v_bc, *up = S.up, *vp = S.vp;
  const double dt = S.dt;
  launch3d(S.s, S.Isq, S.Ieq, S.js, S.je, S.nz, [=] __device__(int I, int j, int k) {
    const long n = g.u3(I, j, k);
    double a = (CAu[n] + PFu[n]);
    if (inviscid) a = (a == 0.0) ? 0.0 : a; else a = a + diffu[n];
    u_bc[n] = a;
    if (u0) up[n] = g.mask2dCu[g.u2(I, j)] * (u0[n] + dt * a);
  });
  launch3d(S.s, S.is, S.ie, S.Jsq, S.Jeq, S.nz, [=] __device__(int i, int J, int k) {
    const long n = g.v3(i, J, k);
    double a = (CAv[n] + PFv[n]);
    if (inviscid) a = (a == 0.0) ? 0.0 : a; else a = a + diffv[n];
    v_bc[n] = a;
    if (v0) vp[n] = g.mask2dCv[g.v2(i, J)] * (v0[n] + dt * a);
  });
}
// uo = mask*(ui + dtx*(u_bc_accel [+ u_accel_bt])) and its v twin (:582-589, :667-676, :930-939); uo may be ui (a point reads itself).
// v_first: which of the two launches goes first at the site, as it always has.
void vel_increment(const StepCall &S, double *uo, double *vo, const double *ui, const double *vi, double dtx, bool with_bt, bool v_first) {
  const m6::GridDev g = S.g;
  const double *u_bc = S.u_bc, *v_bc = S.v_bc, *abu = S.cs->u_accel_bt, *abv = S.cs->v_accel_bt;
  auto v_sweep = [&] {
    launch3d(S.s, S.is, S.ie, S.Jsq, S.Jeq, S.nz, [=] __device__(int i, int J, int k) {
      const long n = g.v3(i, J, k);
      vo[n] = g.mask2dCv[g.v2(i, J)] * (vi[n] + dtx * (with_bt ? (v_bc[n] + abv[n]) : v_bc[n]));
    });
  };
  if (v_first) v_sweep();
  launch3d(S.s, S.Isq, S.Ieq, S.js, S.je, S.nz, [=] __device__(int I, int j, int k) {
    const long n = g.u3(I, j, k);
    uo[n] = g.mask2dCu[g.u2(I, j)] * (ui[n] + dtx * (with_bt ? (u_bc[n] + abu[n]) : u_bc[n]));
  });
  if (!v_first) v_sweep();
}
// out = 0.5*(a + b) on h points (:785-787, :1038-1040, :1581); out may be a
void mean_h(hipStream_t s, const m6::GridDev &gd, double *out, const double *a, const double *b, int i0, int i1, int j0, int j1) {
  const m6::GridDev g = gd;
  launch3d(s, i0, i1, j0, j1, g.nk, [=] __device__(int i, int j, int k) {
    const long n = g.h3(i, j, k);
    out[n] = 0.5 * (a[n] + b[n]);
  });
}
void mean_h(const StepCall &S, double *out, const double *a, const double *b, int i0, int i1, int j0, int j1) {
  mean_h(S.s, S.g, out, a, b, i0, i1, j0, j1);
}
// out = a on h points (:422, :1000)
void copy_h(const StepCall &S, double *out, const double *a, int i0, int i1, int j0, int j1) {
  const m6::GridDev g = S.g;
  launch3d(S.s, i0, i1, j0, j1, S.nz, [=] __device__(int i, int j, int k) { out[g.h3(i, j, k)] = a[g.h3(i, j, k)]; });
}
// uhtr = uhtr + uh*dt, vhtr = vhtr + vh*dt (:1046-1053): cell rows ja..jb, v-face rows Ja..Jb
void accumulate_transports(const StepCall &S, int ja, int jb, int Ja, int Jb) {
  const m6::GridDev g = S.g;
  double *uhtr = S.uhtr, *vhtr = S.vhtr;
  const double *uh = S.uh, *vh = S.vh;
  const double dt = S.dt;
  launch3d(S.s, S.Isq - 2, S.Ieq + 2, ja, jb, S.nz, [=] __device__(int I, int j, int k) {
    const long n = g.u3(I, j, k);
    uhtr[n] = uhtr[n] + uh[n] * dt;
  });
  launch3d(S.s, S.is - 2, S.ie + 2, Ja, Jb, S.nz, [=] __device__(int i, int J, int k) {
    const long n = g.v3(i, J, k);
    vhtr[n] = vhtr[n] + vh[n] * dt;
  });
}
// eta = eta_pred (:918)
void take_eta_pred(const StepCall &S) {
  const m6::GridDev g = S.g;
  double *eta = S.cs->eta;
  const double *eta_pred = S.eta_pred;
  launch3d(S.s, S.is, S.ie, S.js, S.je, 1, [=] __device__(int i, int j, int) { eta[g.h2(i, j)] = eta_pred[g.h2(i, j)]; });
}
// eta = -Z_to_H*bathyT + sum of h (:1521-1535)
void set_eta_from_h(hipStream_t s, const m6::GridDev &gd, double *eta, const double *h) {
  const m6::GridDev g = gd;
  const double Z_to_H = g.Z_to_H;
  const long hstr = (long)g.nih * g.njh;
  const int nz = g.nk;
  launch3d(s, g.isc, g.iec, g.jsc, g.jec, 1, [=] __device__(int i, int j, int) {
    const long n = g.h2(i, j);
    double e = -Z_to_H * g.bathyT[n];
    for (int k = 0; k < nz; k++) e = e + h[n + hstr * k];
    eta[n] = e;
  });
}
// visc_rem_u = visc_rem_v = 1 on the data domain
void set_visc_rem_one(hipStream_t s, const m6::GridDev &gd, double *vru, double *vrv) {
  const m6::GridDev g = gd;
  launch3d(s, g.isd - 1, g.ied, g.jsd, g.jed, g.nk, [=] __device__(int i, int j, int k) { vru[g.u3(i, j, k)] = 1.0; });
  launch3d(s, g.isd, g.ied, g.jsd - 1, g.jed, g.nk, [=] __device__(int i, int j, int k) { vrv[g.v3(i, j, k)] = 1.0; });
}

// ---- the operators the steppers call more than once, each call written once.  Where an entry has an _obc twin that it only forwards to
// with a null OBC, the twin is called with S.OBC. -----------------------------------------------------------------------------------
constexpr int D = MOM6HIP_MEM_DEVICE;

int pressure_force(const StepCall &S) {      // :495, and the eta of the starting pressure :497-503
  const mom6hip_dyn_split_rk2_cs_t *cs = S.cs;
  return mom6hip_pressureforce_fv_bouss(S.ctx, cs->PressureForce_CSp, cs->eqn_of_state, S.h, S.T, S.Sal, step_p_surf(cs), cs->PFu, cs->PFv, cs->pbce,
                                        cs->eta_PF, D);
}
int coradcalc(const StepCall &S, double *CAu, double *CAv) {
  return mom6hip_coradcalc_obc(S.ctx, S.cs->CoriolisAdv, S.OBC, S.u_av, S.v_av, S.cs->h_av, S.uh, S.vh, CAu, CAv, D);
}
int btcalc(const StepCall &S, const double *h_u, const double *h_v) {
  return mom6hip_btcalc_obc(S.ctx, S.BT, S.h, h_u, h_v, 0, S.OBC, D);
}
// the continuity of the predictor and of the corrector: the barotropic transports in, the corrected velocities out in u_av, v_av
int continuity_with_bt(const StepCall &S, const double *u, const double *v, double *h_out, const mom6hip_bt_cont_t *BTC, double *du_cor, double *dv_cor) {
  const mom6hip_dyn_split_rk2_cs_t *cs = S.cs;
  return mom6hip_continuity_obc(S.ctx, cs->continuity_CSp, S.OBC, u, v, S.h, h_out, S.uh, S.vh, S.dt, cs->uhbt, cs->vhbt, cs->visc_rem_u, cs->visc_rem_v,
                                S.u_av, S.v_av, BTC, du_cor, dv_cor, D);
}
// the continuity for uh_in, vh_in and BT_cont (:634-644)
int continuity_for_bt(const StepCall &S) {
  const mom6hip_dyn_split_rk2_cs_t *cs = S.cs;
  return mom6hip_continuity_obc(S.ctx, cs->continuity_CSp, S.OBC, S.u_inst, S.v_inst, S.h, S.hp, S.uh_in, S.vh_in, S.dt, nullptr, nullptr, cs->visc_rem_u,
                                cs->visc_rem_v, nullptr, nullptr, S.BTC, nullptr, nullptr, D);
}
// set_viscous_ML :592 (DYNAMIC_VISCOUS_ML), with the step's starting velocities; part of the library's own vertical viscosity (the hook of
// that seam stands for set_viscous_ML too).  The OBC acts there under ice shelves only.
int viscous_ml(const StepCall &S, const double *u, const double *v) {
  const mom6hip_dyn_split_rk2_cs_t *cs = S.cs;
  if (!S.VV || (S.hk && S.hk->visc_remnant_pred) || !(cs->set_visc_CSp && cs->set_visc_CSp->dynamic_viscous_ML)) return 0;
  M6_REQUIRE(cs->visc && cs->visc->ustar && cs->visc->nkml_visc_u && cs->visc->nkml_visc_v,
             "%s: DYNAMIC_VISCOUS_ML needs forces%%ustar (visc->ustar) and visc%%nkml_visc_u / nkml_visc_v", S.who);
  return m6::set_viscous_ML_dev(S.ctx, cs->set_visc_CSp, u, v, S.h, S.T, S.Sal, cs->eqn_of_state, S.taux, S.tauy, cs->visc->ustar,
                                (double *)cs->visc->nkml_visc_u, (double *)cs->visc->nkml_visc_v, S.dt);
}
// vertvisc_coef, [vertvisc,] vertvisc_remnant (:598-600 without an update; :717-744, :974-994 with one): the host's hook of the seam, else
// the library's own -- through the entries that take the OBC where one is associated, else in one call that can form the velocity
// increment `inc` in its coefficient sweep and share the KV_ML_INVZ2 profile between the calls of a step (`kv`).
int vertvisc_or_hook(const StepCall &S, double *uu, double *vv, double dtx, int update, const m6::VelIncrement *inc, m6::KvmlProfile kv) {
  const mom6hip_dyn_split_rk2_cs_t *cs = S.cs;
  if (!update && S.hk && S.hk->visc_remnant_pred) {
    M6_HIP(hipStreamSynchronize(S.s));
    M6_REQUIRE(S.hk->visc_remnant_pred(S.hk->user, uu, vv, S.h, dtx, cs->visc_rem_u, cs->visc_rem_v) == 0, "visc_remnant_pred hook failed");
    return 0;
  }
  if (update && S.hk && S.hk->vertvisc) {
    M6_HIP(hipStreamSynchronize(S.s));
    M6_REQUIRE(S.hk->vertvisc(S.hk->user, uu, vv, S.h, dtx, cs->visc_rem_u, cs->visc_rem_v) == 0, "vertvisc hook failed");
    return 0;
  }
  if (!S.VV) return 0;
  if (!S.OBC)
    return m6::vertvisc_step_inc(S.ctx, S.VV, uu, vv, S.h, nullptr, update ? S.taux : nullptr, update ? S.tauy : nullptr, cs->visc, dtx, update, nullptr,
                                 nullptr, cs->visc_rem_u, cs->visc_rem_v, inc, D, kv);
  CALL(mom6hip_vertvisc_coef_obc(S.ctx, S.VV, uu, vv, S.h, nullptr, cs->visc, dtx, S.OBC, D));
  if (update) CALL(mom6hip_vertvisc_obc(S.ctx, S.VV, uu, vv, S.h, S.taux, S.tauy, cs->visc, dtx, nullptr, nullptr, S.OBC, D));
  return mom6hip_vertvisc_remnant(S.ctx, S.VV, cs->visc, cs->visc_rem_u, cs->visc_rem_v, dtx, D);
}
// horizontal_viscosity (:860; hu_cont, hv_cont = BT_cont%h_u, %h_v: read only with USE_CONT_THICKNESS): the library's own, with the
// OBC where one is associated, else the host's hook
int hor_visc_or_hook(const StepCall &S) {
  const mom6hip_dyn_split_rk2_cs_t *cs = S.cs;
  const double *hu = S.BTC ? S.BTC->h_u : nullptr, *hv = S.BTC ? S.BTC->h_v : nullptr;
  if (cs->hor_visc && S.OBC) {
    CALL(mom6hip_horizontal_viscosity_obc(S.ctx, cs->hor_visc, S.u_av, S.v_av, cs->h_av, cs->diffu, cs->diffv, S.dt, hu, hv, S.OBC, D));
  } else if (cs->hor_visc) {
    if (m6::horizontal_viscosity_dev(S.ctx, cs->hor_visc, S.u_av, S.v_av, cs->h_av, cs->diffu, cs->diffv, hu, hv)) return 1;
  } else if (S.hk && S.hk->horizontal_viscosity) {
    M6_HIP(hipStreamSynchronize(S.s));
    M6_REQUIRE(S.hk->horizontal_viscosity(S.hk->user, S.u_av, S.v_av, cs->h_av, cs->diffu, cs->diffv) == 0, "horizontal_viscosity hook failed");
  }
  return 0;
}
// btstep (:655, :911; uh0 .. v0: the layer fluxes and their velocities or null, eta_av: null in the predictor)
int step_btstep(const StepCall &S, const double *uh0, const double *vh0, const double *u0, const double *v0, double *eta_av) {
  const mom6hip_dyn_split_rk2_cs_t *cs = S.cs;
  return mom6hip_btstep_obc(S.ctx, S.BT, S.u_inst, S.v_inst, cs->eta, S.dt, S.u_bc, S.v_bc, S.taux, S.tauy, S.RZ_to_H, cs->pbce, cs->eta_PF, S.u_av, S.v_av,
                            cs->u_accel_bt, cs->v_accel_bt, S.eta_pred, cs->uhbt, cs->vhbt, cs->visc_rem_u, cs->visc_rem_v, S.BTC, S.eta_PF_start, nullptr,
                            nullptr, uh0, vh0, u0, v0, eta_av, S.OBC, D);
}
// radiation_open_bdry_conds (:770, :1033) against the velocities the step started with
int radiation(const StepCall &S, double *u, double *v, double dtx) {
  const mom6hip_obc_t *OBC = S.OBC;
  return mom6hip_radiation_open_bdry_conds(S.ctx, OBC, OBC->gamma_uv, OBC->rx_max, OBC->rx_normal, OBC->ry_normal, u, S.u_old, v, S.v_old, dtx, D);
}

// ---- the three steppers: the reference's sequence of calls, built from the pieces above ------------------------------------------------

// step_MOM_dyn_split_RK2 with CS%OBC associated: the reference's sequence of calls one after the other, every operator through its entry
// point with the OBC (regional grids are small: no fused sweeps, no work around the passes in flight), plus the step's own lines for
// the open boundaries: the starting velocities of the radiation (:444-456), open_boundary_zero_normal_flow on the accelerations
// (:565-567, :887-889), radiation_open_bdry_conds on u_av (:765-775) and u_inst (:1030-1034).
// (an associated OBC on several tiles: every tile holds the segments clipped to its data domain, as open_boundary_config leaves them on a PE;
// tests/test_domains.py::test_rk2_step_with_open_boundaries_layout_independence)
int step_with_obc(StepCall &S) {
  mom6hip_ctx_t *ctx = S.ctx;
  mom6hip_dyn_split_rk2_cs_t *cs = S.cs;
  const mom6hip_bt_cont_t *BTC = S.BTC;
  const int is = S.is, ie = S.ie, js = S.js, je = S.je, nz = S.nz;
  double *u_inst = S.u_inst, *v_inst = S.v_inst, *u_av = S.u_av, *v_av = S.v_av, *h = S.h, *uh = S.uh, *vh = S.vh, *h_av = cs->h_av;
  M6_REQUIRE(!S.hk, "step_MOM_dyn_split_RK2: host-side parameterisations (hooks) are not provided with an associated OBC");
  CALL(step_scratch(S, 3));                                                                          // :336-369, :419-421
  double *up = S.up, *vp = S.vp, *hp = S.hp;
  M6_HIP(hipMemcpyAsync(hp, h, S.sz.h3, hipMemcpyDeviceToDevice, S.s));                              // :422
  M6_HIP(hipMemcpyAsync(S.u_old, u_av, S.sz.u3, hipMemcpyDeviceToDevice, S.s));                      // :450-455
  M6_HIP(hipMemcpyAsync(S.v_old, v_av, S.sz.v3, hipMemcpyDeviceToDevice, S.s));

  CALL(pressure_force(S));                                                                           // :495
  CALL(step_eta_PF_start(ctx, cs, &S.eta_PF_start));                                                 // :497-503
  if (!cs->CAu_pred_stored) CALL(coradcalc(S, cs->CAu_pred, cs->CAv_pred));                          // :544-552
  bc_accel(S, cs->CAu_pred, cs->CAv_pred, false, nullptr, nullptr);                                  // :557-564
  CALL(mom6hip_open_boundary_zero_normal_flow(ctx, S.OBC, S.u_bc, S.v_bc, D));                       // :565-567
  vel_increment(S, up, vp, u_inst, v_inst, S.dt, false, true);                                       // :582-589
  CALL(viscous_ml(S, u_inst, v_inst));                                                               // :592
  CALL(vertvisc_or_hook(S, up, vp, S.dt, 0, nullptr, m6::KVML_AS_NOW));                              // :598-600
  CALL(pass(ctx, {{cs->eta, PH | P2D}, {cs->visc_rem_u, PUs}, {cs->visc_rem_v, PVs}}, nz));         // :610-611
  if (!S.BT_cont_BT_thick) CALL(btcalc(S, nullptr, nullptr));                                        // :618
  CALL(mom6hip_bt_mass_source(ctx, S.BT, h, cs->eta, 1, D));
  if (BTC || cs->BT_use_layer_fluxes) {      // :634-644
    CALL(continuity_for_bt(S));
    if (S.BT_cont_BT_thick) CALL(btcalc(S, BTC->h_u, BTC->h_v));
  }
  if (S.calc_dtbt) CALL(mom6hip_set_dtbt_eta(ctx, S.BT, cs->eta, cs->pbce, nullptr, 0.0, 0.0, D));   // :651
  const bool lf = cs->BT_use_layer_fluxes != 0;
  CALL(step_btstep(S, lf ? S.uh_in : nullptr, lf ? S.vh_in : nullptr, lf ? u_inst : nullptr, lf ? v_inst : nullptr, nullptr));   // :655
  vel_increment(S, up, vp, u_inst, v_inst, S.dt_pred, true, true);                                   // :663-676
  CALL(vertvisc_or_hook(S, up, vp, S.dt_pred, 1, nullptr, m6::KVML_AS_NOW));                         // :717-744
  CALL(pass(ctx, {{cs->visc_rem_u, PUs}, {cs->visc_rem_v, PVs}, {up, PU}, {vp, PV}}, nz));          // :747-751
  CALL(continuity_with_bt(S, up, vp, hp, BTC, nullptr, nullptr));                                    // :757
  CALL(pass(ctx, {{hp, PH}, {u_av, PU}, {v_av, PV}, {uh, PU}, {vh, PV}}, nz));                       // :763
  CALL(radiation(S, u_av, v_av, S.dt_pred));                                                         // :770
  mean_h(S, h_av, h, hp, is - 2, ie + 2, js - 2, je + 2);                                            // :785-787
  CALL(mom6hip_bt_mass_source(ctx, S.BT, hp, S.eta_pred, 0, D));                                     // :797
  if (S.BT_cont_BT_thick) CALL(btcalc(S, BTC->h_u, BTC->h_v));                                       // :843
  CALL(hor_visc_or_hook(S));                                                                         // :860
  CALL(coradcalc(S, cs->CAu, cs->CAv));                                                              // :869
  bc_accel(S, cs->CAu, cs->CAv, false, nullptr, nullptr);                                            // :879-886
  CALL(mom6hip_open_boundary_zero_normal_flow(ctx, S.OBC, S.u_bc, S.v_bc, D));                       // :887-889
  CALL(step_btstep(S, lf ? uh : nullptr, lf ? vh : nullptr, lf ? u_av : nullptr, lf ? v_av : nullptr, S.eta_av));   // :911
  take_eta_pred(S);                                                                                  // :918
  vel_increment(S, u_inst, v_inst, u_inst, v_inst, S.dt, true, true);                                // :928-939
  CALL(vertvisc_or_hook(S, u_inst, v_inst, S.dt, 1, nullptr, m6::KVML_AS_NOW));                      // :974-994
  copy_h(S, h_av, h, is - 2, ie + 2, js - 2, je + 2);                                                // :1000
  CALL(pass(ctx, {{cs->visc_rem_u, PUs}, {cs->visc_rem_v, PVs}, {u_inst, PU}, {v_inst, PV}}, nz));  // :1004-1008
  CALL(continuity_with_bt(S, u_inst, v_inst, h, nullptr, nullptr, nullptr));                         // :1015
  CALL(pass(ctx, {{h, PH}, {u_av, PU}, {v_av, PV}, {uh, PU}, {vh, PV}}, nz));                        // :1018, :1027
  CALL(radiation(S, u_inst, v_inst, S.dt));                                                          // :1033
  mean_h(S, h_av, h_av, h, is - 2, ie + 2, js - 2, je + 2);                                          // :1038-1040
  accumulate_transports(S, js - 2, je + 2, S.Jsq - 2, S.Jeq + 2);                                    // :1046-1053
  if (cs->store_CAu) CALL(coradcalc(S, cs->CAu_pred, cs->CAv_pred));                                 // :1055-1069
  cs->CAu_pred_stored = cs->store_CAu ? 1 : 0;
  M6_HIP(hipGetLastError());
  return 0;
}

// step_MOM_dyn_split_RK2 without an OBC: the same sequence with what the closed step allows -- u_bc_accel formed by the kernel that
// produces the later of its terms, the velocity increments formed in the coefficient sweep of the library's vertical viscosity, and
// the group passes in flight behind whatever does not read their halos.
int step_closed(StepCall &S) {
  mom6hip_ctx_t *ctx = S.ctx;
  mom6hip_dyn_split_rk2_cs_t *cs = S.cs;
  const m6::GridDev &g = S.g;
  const mom6hip_bt_cont_t *BTC = S.BTC;
  const mom6hip_visc_hooks_t *hk = S.hk;
  mom6hip_vertvisc_cs_t *VV = S.VV;
  const int is = S.is, ie = S.ie, js = S.js, je = S.je, nz = S.nz, Jsq = S.Jsq, Jeq = S.Jeq;
  double *u_inst = S.u_inst, *v_inst = S.v_inst, *u_av = S.u_av, *v_av = S.v_av, *h = S.h, *uh = S.uh, *vh = S.vh, *h_av = cs->h_av;
  const double dt = S.dt, dt_pred = S.dt_pred;
  M6_REQUIRE(!VV || cs->visc, "step_MOM_dyn_split_RK2: vertvisc_CSp needs the visc argument (cs->visc)");
  CALL(step_scratch(S, 1));                                                                          // :336-369, :419-421
  double *up = S.up, *vp = S.vp, *hp = S.hp, *u_bc = S.u_bc, *v_bc = S.v_bc;
  // hp = h (:422).  The continuity calls at :634 and :757 write every cell of the compute domain (continuity.hip: the convergence of
  // the last direction covers is..ie, js..je) and nothing reads hp before them, so only the frame outside the compute domain is copied:
  // what the calls and pass_hp_uv do not overwrite there keeps h, as in the reference.
  copy_h(S, hp, h, g.isd, g.ied, g.jsd, js - 1); copy_h(S, hp, h, g.isd, g.ied, je + 1, g.jed);
  copy_h(S, hp, h, g.isd, is - 1, js, je); copy_h(S, hp, h, ie + 1, g.ied, js, je);

  // u_bc_accel = (CAu_pred + PFu) + diffu (:557-564) is formed by the kernel that produces the later of its terms: pgf_face_kernel when
  // CAu_pred was stored by the step before, coradcalc_kernel otherwise (mom6hip_ctx::BcAccelFuse); the sweep bc_accel runs only when
  // neither took it (another form of PressureForce) or when the first up, vp are wanted from it (hooks).
  // Without viscosity hooks and hor_visc, diffu = diffv = +0.0 (inviscid); and the first up, vp (:582-589) are only read by vertvisc_coef.
  // The library's own vertical viscosity forms the velocity increments of :582-589, :667-676 and :930-939 inside its coefficient sweep
  // (vv_fused; m6::vertvisc_step_inc: the same expression on the same numbers), so the step's sweeps for them are not launched.
  const bool inviscid = (hk == nullptr) && (cs->hor_visc == nullptr);      // diffu = diffv = 0
  const bool vv_fused = VV && !(hk && (hk->visc_remnant_pred || hk->vertvisc));
  const bool need_up1 = (!inviscid || VV) && !vv_fused;
  // The KV_ML_INVZ2 profile (find_coupling_coef :1873-1886) is a function of the thicknesses and of constants.  The three calls of
  // the step (:598, :717 and :974 of the reference) all pass this h with no dz, and nothing writes h before the continuity of :1015,
  // after the third: the profile is formed by the first and the other two calls read it (kv_first, kv_later).  A hook in place of any of
  // the three calls (vv_fused) or MOM6HIP_VV_KVML_ONCE=0 leaves every call forming its own.
  const bool kv_once = vv_fused && kvml_once();
  const m6::KvmlProfile kv_first = kv_once ? m6::KVML_PRODUCE : m6::KVML_AS_NOW, kv_later = kv_once ? m6::KVML_CONSUME : m6::KVML_AS_NOW;
  mom6hip_ctx::BcAccelFuse fuse1{nullptr, nullptr, cs->diffu, cs->diffv, u_bc, v_bc, inviscid ? 1 : 0, false};
  const bool try_fuse1 = !need_up1;
  if (try_fuse1 && cs->CAu_pred_stored) { fuse1.au = cs->CAu_pred; fuse1.av = cs->CAv_pred; ctx->bc_fuse = &fuse1; }
  const int rc_pf = pressure_force(S);                                                               // :495
  ctx->bc_fuse = nullptr;
  if (rc_pf) return rc_pf;
  CALL(step_eta_PF_start(ctx, cs, &S.eta_PF_start));                                                 // :497-503
  if (!cs->CAu_pred_stored) {   // :544-552
    if (try_fuse1) { fuse1.au = cs->PFu; fuse1.av = cs->PFv; ctx->bc_fuse = &fuse1; }
    const int rc_ca = coradcalc(S, cs->CAu_pred, cs->CAv_pred);
    ctx->bc_fuse = nullptr;
    if (rc_ca) return rc_ca;
  }
  // u_bc_accel = (CAu_pred + PFu) + diffu ; up = mask*(u + dt*u_bc_accel)   :557-564, :582-589
  if (!fuse1.done) bc_accel(S, cs->CAu_pred, cs->CAv_pred, inviscid, need_up1 ? u_inst : nullptr, need_up1 ? v_inst : nullptr);
  CALL(viscous_ml(S, u_inst, v_inst));                                                               // :592
  const m6::VelIncrement inc1{u_inst, v_inst, u_bc, v_bc, nullptr, nullptr, dt};      // up = mask * (u + dt * u_bc_accel) :582-589
  CALL(vertvisc_or_hook(S, up, vp, dt, 0, vv_fused ? &inc1 : nullptr, kv_first));                    // :598-600
  // pass_eta, pass_visc_rem :541 / :607-611 / :631: in flight behind btcalc and bt_mass_source, which read no halo (the reference
  // completes pass_visc_rem at :631 for the same reason: the continuity below forms fluxes in the rows of visc_rem's halo)
  CALL(pass_start(ctx, {{cs->eta, PH | P2D}, {cs->visc_rem_u, PUs}, {cs->visc_rem_v, PVs}}, nz, 0));

  // btcalc, bt_mass_source :627-630 ; continuity for BT_cont and the layer fluxes :634-644
  if (!S.BT_cont_BT_thick) CALL(btcalc(S, nullptr, nullptr));
  CALL(mom6hip_bt_mass_source(ctx, S.BT, h, cs->eta, 1, D));
  if (BTC || cs->BT_use_layer_fluxes) {
    // (this call is made for uh_in, vh_in and BT_cont: the thicknesses it would leave in hp are rewritten by the call at :757 before
    // anything reads them, so the convergence of its second direction is not launched)
    ctx->cont_fluxes_only = true;
    const int rc_c = continuity_around_pass(ctx, [&]() -> int { return continuity_for_bt(S); });
    ctx->cont_fluxes_only = false;
    if (rc_c) return rc_c;
    if (S.BT_cont_BT_thick) CALL(btcalc(S, BTC->h_u, BTC->h_v));
  } else {
    CALL(m6::complete_group_pass(ctx));
  }
  if (S.calc_dtbt) CALL(mom6hip_set_dtbt_eta(ctx, S.BT, cs->eta, cs->pbce, nullptr, 0.0, 0.0, D));   // :651
  const bool lf = cs->BT_use_layer_fluxes != 0;
  CALL(step_btstep(S, lf ? S.uh_in : nullptr, lf ? S.vh_in : nullptr, lf ? u_inst : nullptr, lf ? v_inst : nullptr, nullptr));   // :655

  // up = u + dt_pred*(u_bc_accel + u_accel_bt) :663-676 ; vertvisc_coef, vertvisc, vertvisc_remnant :717-744
  if (!vv_fused) vel_increment(S, up, vp, u_inst, v_inst, dt_pred, true, true);
  const m6::VelIncrement inc2{u_inst, v_inst, u_bc, v_bc, cs->u_accel_bt, cs->v_accel_bt, dt_pred};
  CALL(vertvisc_or_hook(S, up, vp, dt_pred, 1, vv_fused ? &inc2 : nullptr, kv_later));
  // pass_visc_rem, pass_uvp :741-751 in flight behind the continuity's own rows (continuity_around_pass)
  CALL(pass_start(ctx, {{cs->visc_rem_u, PUs}, {cs->visc_rem_v, PVs}, {up, PU}, {vp, PV}}, nz, 1));
  CALL(continuity_around_pass(ctx, [&]() -> int { return continuity_with_bt(S, up, vp, hp, BTC, nullptr, nullptr); }));   // :757
  // pass_hp_uv :763 in flight behind bt_mass_source and btcalc (no halos) and behind the rows of h_av, horizontal_viscosity and
  // CorAdCalc that lie at least a halo width inside the tile; the rows along the two edges follow the completion
  const bool hv_hook = !cs->hor_visc && hk && hk->horizontal_viscosity;
  auto after_hp_uv = [&]() -> int {      // (pure functions of their inputs, row by row: a row computed twice gets the same bits)
    const m6::GridDev w = ctx->g;      // the window
    mean_h(S, h_av, h, hp, is - 2, ie + 2, w.jsc - 2, w.jec + 2);                                     // :785-787
    if (cs->hor_visc) {   // :860 (hu_cont, hv_cont = BT_cont%h_u, %h_v: read only with USE_CONT_THICKNESS)
      if (m6::horizontal_viscosity_dev(ctx, cs->hor_visc, u_av, v_av, h_av, cs->diffu, cs->diffv, BTC ? BTC->h_u : nullptr,
                                       BTC ? BTC->h_v : nullptr)) return 1;
    }
    if (!hv_hook) CALL(coradcalc(S, cs->CAu, cs->CAv));                                               // :869
    return 0;
  };
  CALL(pass_start(ctx, {{hp, PH}, {u_av, PU}, {v_av, PV}, {uh, PU}, {vh, PV}}, nz, 2));             // :763
  CALL(mom6hip_bt_mass_source(ctx, S.BT, hp, S.eta_pred, 0, D));                                     // :797
  if (S.BT_cont_BT_thick) CALL(btcalc(S, BTC->h_u, BTC->h_v));                                       // :843
  // u_bc_accel = (CAu + PFu) + diffu (:879-886) formed by coradcalc_kernel, row window by row window (diffu of a row is complete
  // before CorAdCalc of that row is launched)
  mom6hip_ctx::BcAccelFuse fuse2{cs->PFu, cs->PFv, cs->diffu, cs->diffv, u_bc, v_bc, inviscid ? 1 : 0, false};
  ctx->bc_fuse = &fuse2;
  int rc_ap = around_pass(ctx, after_hp_uv);
  // (the hook of :860 is left as it stands, not through hor_visc_or_hook: bc_fuse has to be taken back on every way out, and a hook
  // that fails here has always returned 1)
  if (rc_ap == 0 && hv_hook) {
    rc_ap = hipStreamSynchronize(S.s) == hipSuccess ? 0 : 1;
    if (rc_ap == 0 && hk->horizontal_viscosity(hk->user, u_av, v_av, h_av, cs->diffu, cs->diffv) != 0) {
      m6::set_error("horizontal_viscosity hook failed"); rc_ap = 1;
    }
    if (rc_ap == 0) rc_ap = coradcalc(S, cs->CAu, cs->CAv);                                           // :869
  }
  ctx->bc_fuse = nullptr;
  if (rc_ap) return rc_ap;
  if (!fuse2.done) bc_accel(S, cs->CAu, cs->CAv, inviscid, nullptr, nullptr);                        // :879-886
  CALL(step_btstep(S, lf ? uh : nullptr, lf ? vh : nullptr, lf ? u_av : nullptr, lf ? v_av : nullptr, S.eta_av));   // :911
  take_eta_pred(S);                                                                                  // :918
  // u = u + dt*(u_bc_accel + u_accel_bt) :928-939 (in place) ; vertvisc_coef, vertvisc, vertvisc_remnant :974-994
  if (!vv_fused) vel_increment(S, u_inst, v_inst, u_inst, v_inst, dt, true, false);
  const m6::VelIncrement inc3{u_inst, v_inst, u_bc, v_bc, cs->u_accel_bt, cs->v_accel_bt, dt};
  CALL(vertvisc_or_hook(S, u_inst, v_inst, dt, 1, vv_fused ? &inc3 : nullptr, kv_later));
  copy_h(S, h_av, h, is - 2, ie + 2, js - 2, je + 2);                                                // :1000
  CALL(pass_start(ctx, {{cs->visc_rem_u, PUs}, {cs->visc_rem_v, PVs}, {u_inst, PU}, {v_inst, PV}}, nz, 3));     // :991-1008
  CALL(continuity_around_pass(ctx, [&]() -> int { return continuity_with_bt(S, u_inst, v_inst, h, nullptr, nullptr, nullptr); }));   // :1015
  // pass_h, pass_av_uvh :1018-1043 in flight behind the rows of the three accumulations and of CorAdCalc that need no halo row.
  // The accumulations work in place: their rows are split exactly (inner rows before the completion, the two edge bands after).
  auto accumulate = [&](int ja, int jb, int Ja, int Jb) {      // cell rows ja..jb, v-face rows Ja..Jb
    mean_h(S, h_av, h_av, h, is - 2, ie + 2, ja, jb);                                                 // :1038-1040
    accumulate_transports(S, ja, jb, Ja, Jb);                                                         // :1046-1053
  };
  auto next_CA = [&]() -> int {
    if (cs->store_CAu) CALL(coradcalc(S, cs->CAu_pred, cs->CAv_pred));                                // :1055-1069
    return 0;
  };
  CALL(pass_start(ctx, {{h, PH}, {u_av, PU}, {v_av, PV}, {uh, PU}, {vh, PV}}, nz, 4));               // :1018, :1027
  if (split_rows(ctx)) {
    ctx->overlap[0]++;
    const int W = is - g.isd;      // the halo width: CorAdCalc's rows at least W inside the tile read rows of the compute domain only
    accumulate(js + 2, je - 2, Jsq + 2, Jeq - 2);      // (h_av's inner rows reach two rows beyond the window of next_CA below)
    m6::row_window(ctx, js + W + 2, je - W - 2);
    int rc = next_CA();
    m6::row_window_reset(ctx);
    if (rc) { m6::ErrorKeeper keep; m6::complete_group_pass(ctx); return rc; }
    CALL(m6::complete_group_pass(ctx));
    accumulate(js - 2, js + 1, Jsq - 2, Jsq + 1);
    accumulate(je - 1, je + 2, Jeq - 1, Jeq + 2);
    m6::row_window(ctx, js, js + W + 1);
    rc = next_CA();
    if (!rc) { m6::row_window(ctx, je - W - 1, je); rc = next_CA(); }
    m6::row_window_reset(ctx);
    if (rc) return rc;
  } else {
    ctx->overlap[2]++;
    CALL(m6::complete_group_pass(ctx));
    accumulate(js - 2, je + 2, Jsq - 2, Jeq + 2);
    CALL(next_CA());
  }
  cs->CAu_pred_stored = cs->store_CAu ? 1 : 0;
  M6_HIP(hipGetLastError());
  return 0;
}

// ---- SPLIT_RK2B: src/core/MOM_dynamics_split_RK2b.F90 ----------------------------------------------------------
// The same operators in another order: the step starts from the filtered velocities u_av, v_av (the model's prognostic
// velocities in this scheme), does a first continuity + CorAdCalc + horizontal_viscosity with them, rebuilds the
// instantaneous velocities from the stored barotropic increments (:641-646) and ends with the increments the final
// continuity returns (du_cor, dv_cor :979-981).  cs->u_av, cs->v_av, cs->h_av are the step's u_inst, v_inst, h_av.
// CS%OBC: the OBC entry points of the operators, open_boundary_zero_normal_flow on the accelerations (:571-573, :866-868) and
// radiation_open_bdry_conds on u_av (:766-774, :1000-1002), as in step_with_obc.
int step_rk2b(StepCall &S) {
  mom6hip_ctx_t *ctx = S.ctx;
  mom6hip_dyn_split_rk2_cs_t *cs = S.cs;
  const m6::GridDev g = S.g;
  const mom6hip_obc_t *OBC = S.OBC;
  const mom6hip_bt_cont_t *BTC = S.BTC;
  const mom6hip_visc_hooks_t *hk = S.hk;
  mom6hip_vertvisc_cs_t *VV = S.VV;
  const int is = S.is, ie = S.ie, js = S.js, je = S.je, nz = S.nz;
  double *u_inst = S.u_inst, *v_inst = S.v_inst, *u_av = S.u_av, *v_av = S.v_av, *h = S.h, *uh = S.uh, *vh = S.vh, *h_av = cs->h_av;
  M6_REQUIRE(!OBC || !hk, "step_MOM_dyn_split_RK2b: host-side parameterisations (hooks) are not provided with an associated OBC");
  M6_REQUIRE(!VV || cs->visc, "step_MOM_dyn_split_RK2b: vertvisc_CSp needs the visc argument (cs->visc)");
  // up = vp = u_inst = v_inst = 0 (:404) matters only at the halo faces beyond a closed edge, which nothing writes: up, vp are
  // zeroed by the rule of step_scratch, u_inst, v_inst by dyn_split_rk2b_init.
  CALL(step_scratch(S, 2));
  double *up = S.up, *vp = S.vp, *hp = S.hp;
  M6_HIP(hipMemcpyAsync(hp, h, S.sz.h3, hipMemcpyDeviceToDevice, S.s));                              // :403
  if (OBC) {                                                                                          // :436-442
    M6_HIP(hipMemcpyAsync(S.u_old, u_av, S.sz.u3, hipMemcpyDeviceToDevice, S.s));
    M6_HIP(hipMemcpyAsync(S.v_old, v_av, S.sz.v3, hipMemcpyDeviceToDevice, S.s));
  }
  // The KV_ML_INVZ2 profile is formed by the first of the step's three calls (:604, :724, :946) and read by the other two, as in
  // step_MOM_dyn_split_RK2 above: all three pass this h with no dz, and h is first written by the continuity of :979.  Not with a hook
  // in place of one of the calls, nor through the separate entries an OBC takes.
  const bool kv_once = VV && !OBC && !(hk && (hk->visc_remnant_pred || hk->vertvisc)) && kvml_once();
  const m6::KvmlProfile kv_first = kv_once ? m6::KVML_PRODUCE : m6::KVML_AS_NOW, kv_later = kv_once ? m6::KVML_CONSUME : m6::KVML_AS_NOW;

  // continuity with the filtered velocities :488, PressureForce :498, pass_hp_uhvh :535, h_av :540-542
  CALL(mom6hip_continuity_obc(ctx, cs->continuity_CSp, OBC, u_av, v_av, h, hp, uh, vh, S.dt, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                              nullptr, nullptr, nullptr, D));
  CALL(pressure_force(S));
  CALL(step_eta_PF_start(ctx, cs, &S.eta_PF_start));                                                 // :497-503
  CALL(pass(ctx, {{hp, PH}, {uh, PU}, {vh, PV}}, nz));
  mean_h(S, h_av, h, hp, is - 2, ie + 2, js - 2, je + 2);
  CALL(coradcalc(S, cs->CAu_pred, cs->CAv_pred));                                                     // :548
  CALL(hor_visc_or_hook(S));                                                                          // :555

  // u_bc_accel :561-568 ; up = mask*(u_av + dt*u_bc_accel) :587-594 (read only by vertvisc_coef), in the same sweep without an OBC,
  // after the accelerations are zeroed on the segments with one
  const bool need_up = VV || (hk && hk->visc_remnant_pred);
  bc_accel(S, cs->CAu_pred, cs->CAv_pred, false, need_up && !OBC ? u_av : nullptr, need_up && !OBC ? v_av : nullptr);
  if (OBC) {
    CALL(mom6hip_open_boundary_zero_normal_flow(ctx, OBC, S.u_bc, S.v_bc, D));                        // :571-573
    if (VV) vel_increment(S, up, vp, u_av, v_av, S.dt, false, false);                                 // :587-594
  }
  CALL(viscous_ml(S, u_av, v_av));                                                                    // :598
  CALL(vertvisc_or_hook(S, up, vp, S.dt, 0, nullptr, kv_first));                                      // :598-606
  CALL(pass(ctx, {{cs->eta, PH | P2D}, {cs->visc_rem_u, PUs}, {cs->visc_rem_v, PVs}}, nz));          // :616-617
  if (!S.BT_cont_BT_thick) CALL(btcalc(S, nullptr, nullptr));                                         // :623-625
  CALL(mom6hip_bt_mass_source(ctx, S.BT, h, cs->eta, 1, D));
  {   // the instantaneous velocities :641-646, pass_uv_inst :648
    const double *du = cs->du_av_inst, *dv = cs->dv_av_inst, *vru = cs->visc_rem_u, *vrv = cs->visc_rem_v;
    launch3d(S.s, S.Isq, S.Ieq, js, je, nz, [=] __device__(int I, int j, int k) {
      const long n = g.u3(I, j, k);
      u_inst[n] = u_av[n] - du[g.u2(I, j)] * vru[n];
    });
    launch3d(S.s, is, ie, S.Jsq, S.Jeq, nz, [=] __device__(int i, int J, int k) {
      const long n = g.v3(i, J, k);
      v_inst[n] = v_av[n] - dv[g.v2(i, J)] * vrv[n];
    });
  }
  CALL(pass(ctx, {{u_inst, PU}, {v_inst, PV}}, nz));
  CALL(continuity_for_bt(S));                                                                         // :652
  if (S.BT_cont_BT_thick) CALL(btcalc(S, BTC->h_u, BTC->h_v));                                        // :655-658
  if (S.calc_dtbt) CALL(mom6hip_set_dtbt_eta(ctx, S.BT, cs->eta, cs->pbce, nullptr, 0.0, 0.0, D));    // :664
  CALL(step_btstep(S, S.uh_in, S.vh_in, u_inst, v_inst, nullptr));                                    // :668

  vel_increment(S, up, vp, u_inst, v_inst, S.dt_pred, true, true);                                    // :675-686
  CALL(vertvisc_or_hook(S, up, vp, S.dt_pred, 1, nullptr, kv_later));                                 // :724-745
  // pass_visc_rem, pass_uvp :748, :752 in flight behind the continuity's own rows, as in the RK2 stepping (continuity_around_pass)
  CALL(pass_start(ctx, {{cs->visc_rem_u, PUs}, {cs->visc_rem_v, PVs}, {up, PU}, {vp, PV}}, nz, 1));
  if (OBC) {
    CALL(m6::complete_group_pass(ctx));
    CALL(continuity_with_bt(S, up, vp, hp, BTC, nullptr, nullptr));
  } else {
    CALL(continuity_around_pass(ctx, [&]() -> int { return continuity_with_bt(S, up, vp, hp, BTC, nullptr, nullptr); }));   // :758
  }
  CALL(pass(ctx, {{hp, PH}, {u_av, PU}, {v_av, PV}, {uh, PU}, {vh, PV}}, nz));                      // :764
  if (OBC) CALL(radiation(S, u_av, v_av, S.dt_pred));                                                 // :770
  mean_h(S, h_av, h, hp, is - 2, ie + 2, js - 2, je + 2);                                             // :780-782
  CALL(mom6hip_bt_mass_source(ctx, S.BT, hp, S.eta_pred, 0, D));                                      // :790
  if (S.BT_cont_BT_thick) CALL(btcalc(S, BTC->h_u, BTC->h_v));                                        // :824-827
  CALL(hor_visc_or_hook(S));                                                                          // :841
  CALL(coradcalc(S, cs->CAu, cs->CAv));                                                               // :848
  bc_accel(S, cs->CAu, cs->CAv, false, nullptr, nullptr);                                             // :854-861
  if (OBC) CALL(mom6hip_open_boundary_zero_normal_flow(ctx, OBC, S.u_bc, S.v_bc, D));                 // :866-868
  CALL(step_btstep(S, uh, vh, u_av, v_av, S.eta_av));                                                 // :889
  take_eta_pred(S);                                                                                   // :898
  vel_increment(S, u_inst, v_inst, u_inst, v_inst, S.dt, true, false);                                // :908-919
  CALL(vertvisc_or_hook(S, u_inst, v_inst, S.dt, 1, nullptr, kv_later));                              // :946-963
  CALL(pass_start(ctx, {{cs->visc_rem_u, PUs}, {cs->visc_rem_v, PVs}, {u_inst, PU}, {v_inst, PV}}, nz, 3));     // :967, :971
  if (OBC) {
    CALL(m6::complete_group_pass(ctx));
    CALL(continuity_with_bt(S, u_inst, v_inst, h, nullptr, cs->du_av_inst, cs->dv_av_inst));
  } else {
    CALL(continuity_around_pass(ctx, [&]() -> int { return continuity_with_bt(S, u_inst, v_inst, h, nullptr, cs->du_av_inst, cs->dv_av_inst); }));   // :979
  }
  CALL(pass(ctx, {{h, PH}, {u_av, PU}, {v_av, PV}, {uh, PU}, {vh, PV}}, nz));                        // :993
  if (OBC) CALL(radiation(S, u_av, v_av, S.dt));                                                      // :1001
  accumulate_transports(S, js - 2, je + 2, S.Jsq - 2, S.Jeq + 2);                                     // :1004-1011
  M6_HIP(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" {

int mom6hip_dyn_split_rk2_init(mom6hip_ctx_t *ctx, mom6hip_dyn_split_rk2_cs_t *cs, const double *u, const double *v, const double *h,
                               double *uh, double *vh, double dt) {
  M6_REQUIRE(ctx && u && v && h && uh && vh, "dyn_split_rk2_init: null argument");
  CALL(check(cs, "dyn_split_rk2_init"));
  const m6::GridDev g = ctx->g;
  const Sz sz = sizes(g);
  hipStream_t s = ctx->stream;
  set_eta_from_h(s, g, cs->eta, h);                                                                  // :1521-1535
  M6_HIP(hipMemsetAsync(cs->diffu, 0, sz.u3, s)); M6_HIP(hipMemsetAsync(cs->diffv, 0, sz.v3, s));
  if (cs->hor_visc) {   // :1543-1550 (with the velocities and thicknesses of the call, not u_av and h_av)
    const mom6hip_bt_cont_t *B = cs->BT_cont;
    M6_REQUIRE(cs->hor_visc->initialized, "MOM_hor_visc: Module must be initialized before it is used.");
    if (cs->OBC) CALL(mom6hip_horizontal_viscosity_obc(ctx, cs->hor_visc, u, v, h, cs->diffu, cs->diffv, dt, B ? B->h_u : nullptr, B ? B->h_v : nullptr, cs->OBC, D));
    else if (m6::horizontal_viscosity_dev(ctx, cs->hor_visc, u, v, h, cs->diffu, cs->diffv, B ? B->h_u : nullptr, B ? B->h_v : nullptr)) return 1;
  } else if (cs->hooks && cs->hooks->horizontal_viscosity) {
    M6_HIP(hipStreamSynchronize(s));
    M6_REQUIRE(cs->hooks->horizontal_viscosity(cs->hooks->user, u, v, h, cs->diffu, cs->diffv) == 0, "horizontal_viscosity hook failed");
  }
  set_visc_rem_one(s, g, cs->visc_rem_u, cs->visc_rem_v);
  M6_HIP(hipMemcpyAsync(cs->u_av, u, sz.u3, hipMemcpyDeviceToDevice, s));     // :1552-1558
  M6_HIP(hipMemcpyAsync(cs->v_av, v, sz.v3, hipMemcpyDeviceToDevice, s));
  // :1560-1610: first transports, h_av and (store_CAu) the predictor's Coriolis terms
  {
    double *h_tmp = cs->CAu;   // free at this point; CAu is rewritten by the first step before it is read
    M6_REQUIRE(sz.u3 >= sz.h3, "dyn_split_rk2_init: internal scratch too small");
    M6_HIP(hipMemcpyAsync(h_tmp, h, sz.h3, hipMemcpyDeviceToDevice, s));
    const double *uu = cs->store_CAu ? cs->u_av : u, *vv = cs->store_CAu ? cs->v_av : v;
    CALL(mom6hip_continuity_obc(ctx, cs->continuity_CSp, cs->OBC, uu, vv, h, h_tmp, uh, vh, dt, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                nullptr, nullptr, nullptr, D));
    CALL(pass(ctx, {{h_tmp, PH}}, g.nk));
    mean_h(s, g, cs->h_av, h, h_tmp, g.isd, g.ied, g.jsd, g.jed);
  }
  if (cs->store_CAu) {
    CALL(pass(ctx, {{cs->u_av, PU}, {cs->v_av, PV}, {uh, PU}, {vh, PV}}, g.nk));
    CALL(mom6hip_coradcalc_obc(ctx, cs->CoriolisAdv, cs->OBC, cs->u_av, cs->v_av, cs->h_av, uh, vh, cs->CAu_pred, cs->CAv_pred, D));
    cs->CAu_pred_stored = 1;
    CALL(pass(ctx, {{cs->u_av, PU}, {cs->v_av, PV}, {cs->CAu_pred, PU}, {cs->CAv_pred, PV}}, g.nk));   // :1615-1622
  } else {
    cs->CAu_pred_stored = 0;
    CALL(pass(ctx, {{cs->u_av, PU}, {cs->v_av, PV}, {cs->h_av, PH}, {uh, PU}, {vh, PV}}, g.nk));
  }
  M6_HIP(hipGetLastError());
  return 0;
}

int mom6hip_step_dyn_split_rk2(mom6hip_ctx_t *ctx, mom6hip_dyn_split_rk2_cs_t *cs, double *u_inst, double *v_inst, double *h,
                               const double *T, const double *S, double dt, const double *taux, const double *tauy, double RZ_to_H,
                               double *uh, double *vh, double *uhtr, double *vhtr, double *eta_av, int32_t calc_dtbt) {
  M6_REQUIRE(ctx && u_inst && v_inst && h && taux && tauy && uh && vh && uhtr && vhtr && eta_av, "step_MOM_dyn_split_RK2: null argument");
  CALL(check(cs, "step_MOM_dyn_split_RK2"));
  M6_REQUIRE(!cs->eqn_of_state || (T && S), "step_MOM_dyn_split_RK2: an equation of state needs tv%%T and tv%%S");
  StepCall C{};
  step_call(C, ctx, cs, "step_MOM_dyn_split_RK2", u_inst, v_inst, cs->u_av, cs->v_av, h, T, S, dt, taux, tauy, RZ_to_H, uh, vh, uhtr, vhtr, eta_av,
            calc_dtbt);
  return cs->OBC ? step_with_obc(C) : step_closed(C);
}

int mom6hip_dyn_split_rk2b_init(mom6hip_ctx_t *ctx, mom6hip_dyn_split_rk2_cs_t *cs, const double *h) {
  M6_REQUIRE(ctx && h, "dyn_split_rk2b_init: null argument");
  CALL(check(cs, "dyn_split_rk2b_init"));
  M6_REQUIRE(cs->du_av_inst && cs->dv_av_inst, "dyn_split_rk2b_init: du_av_inst / dv_av_inst are not allocated");
  const m6::GridDev g = ctx->g;
  const Sz sz = sizes(g);
  hipStream_t s = ctx->stream;
  set_eta_from_h(s, g, cs->eta, h);                                                                  // :1406-1420
  M6_HIP(hipMemsetAsync(cs->diffu, 0, sz.u3, s)); M6_HIP(hipMemsetAsync(cs->diffv, 0, sz.v3, s));       // :1155-1156
  M6_HIP(hipMemsetAsync(cs->du_av_inst, 0, sz.u3 / g.nk, s)); M6_HIP(hipMemsetAsync(cs->dv_av_inst, 0, sz.v3 / g.nk, s));   // :1164-1165
  M6_HIP(hipMemsetAsync(cs->u_av, 0, sz.u3, s)); M6_HIP(hipMemsetAsync(cs->v_av, 0, sz.v3, s));         // u_inst = v_inst = 0 :404
  set_visc_rem_one(s, g, cs->visc_rem_u, cs->visc_rem_v);
  M6_HIP(hipGetLastError());
  return 0;
}

int mom6hip_step_dyn_split_rk2b(mom6hip_ctx_t *ctx, mom6hip_dyn_split_rk2_cs_t *cs, double *u_av, double *v_av, double *h,
                                const double *T, const double *S, double dt, const double *taux, const double *tauy, double RZ_to_H,
                                double *uh, double *vh, double *uhtr, double *vhtr, double *eta_av, int32_t calc_dtbt) {
  M6_REQUIRE(ctx && u_av && v_av && h && taux && tauy && uh && vh && uhtr && vhtr && eta_av, "step_MOM_dyn_split_RK2b: null argument");
  CALL(check(cs, "step_MOM_dyn_split_RK2b"));
  M6_REQUIRE(!cs->eqn_of_state || (T && S), "step_MOM_dyn_split_RK2b: an equation of state needs tv%%T and tv%%S");
  M6_REQUIRE(cs->du_av_inst && cs->dv_av_inst, "step_MOM_dyn_split_RK2b: du_av_inst / dv_av_inst are not allocated");
  StepCall C{};
  step_call(C, ctx, cs, "step_MOM_dyn_split_RK2b", cs->u_av, cs->v_av, u_av, v_av, h, T, S, dt, taux, tauy, RZ_to_H, uh, vh, uhtr, vhtr, eta_av,
            calc_dtbt);
  return step_rk2b(C);
}

}  // extern "C"
