// hordiff_call.hpp -- what tracer_hordiff (tracer_hor_diff.hip) hands to its branches: one record of the call on device arrays, and
// the branches' declarations.  khdt_x, khdt_y and the iteration count are those tracer_hordiff has formed.
#pragma once
#include "common.hpp"

namespace m6 {

// The diagnostics neutral_diffusion and hor_bnd_diffusion post themselves (mom6hip_tracer_mix_diag_t), as device views of the arrays a
// tracer asked for (null: not asked for), in the order of the record
enum { MIX_DFX_2D = 0, MIX_DFY_2D, MIX_DFXY_CONT, MIX_DFXY_CONT_2D, MIX_DFXY_CONC, MIX_HBD_DFX, MIX_HBD_DFY, MIX_HBD_DFX_2D, MIX_HBD_DFY_2D,
       MIX_HBDXY_CONT, MIX_HBDXY_CONT_2D, MIX_HBDXY_CONC, MIX_COUNT };
struct MixDiag { double *a[MIX_COUNT]; };

struct HordiffCall {
  mom6hip_ctx_t *ctx;
  Stager &st;
  const double *h, *khdt_x, *khdt_y;
  int num_itts;
  double I_numitts;
  const std::vector<double *> &d_tr;      // the tracers
  const std::vector<double> &cu;          // their conc_underflow
  int idx_T, idx_S;                       // tv%T and tv%S among them
  const mom6hip_eos_t *eos;
  const double *p_surf, *h_ML;            // null where the call has none
  const double *ebt_struct;               // VarMix%ebt_struct with KHTR_USE_EBT_STRUCT where it is read, null without
  int *halo_updates;
  const MixDiag *mix;                     // one per tracer, or null: no such diagnostic in this call (then num_itts == 1 is not required)
  double Idt;                             // 1.0 / (I_numitts * dt), as neutral_diffusion and hor_bnd_diffusion form it
};

// USE_HORIZONTAL_BOUNDARY_DIFFUSION (hor_bnd_diffusion.hip)
int hbd_branch(const HordiffCall &c, const mom6hip_hor_bnd_diffusion_cs_t *hbd, double KhTr_min, bool full_depth_khtr_min);
// USE_NEUTRAL_DIFFUSION (neutral_diffusion.hip); with nd->unsupported[0] and ndd it is neutral_disc_branch (neutral_diffusion_disc.hip)
int neutral_branch(const HordiffCall &c, const mom6hip_neutral_diffusion_cs_t *nd, const mom6hip_ndiff_discontinuous_cs_t *ndd);
int neutral_disc_branch(const HordiffCall &c, const mom6hip_neutral_diffusion_cs_t *nd, const mom6hip_ndiff_discontinuous_cs_t *ndd);
// DIFFUSE_ML_TO_INTERIOR (epipycnal_diff.hip)
int epipycnal_branch(const HordiffCall &c, const mom6hip_epipycnal_cs_t *epi);

}  // namespace m6
