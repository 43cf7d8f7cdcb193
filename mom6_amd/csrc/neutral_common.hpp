// neutral_common.hpp -- what the two reconstructions of MOM_neutral_diffusion (neutral_diffusion.hip: continuous,
// neutral_diffusion_disc.hip: NDIFF_CONTINUOUS = False) share: the state of the faces that their surface, flux and update kernels hand
// to each other, a lane's face or column, the layer the surface boundary layer ends in (hor_bnd_diffusion.hip reads that too), what a
// dry face holds, the store of a layer's tendency, and the host driver of neutral_diffusion's outer structure.
#pragma once
#include <functional>
#include <vector>

#include "hordiff_call.hpp"

namespace m6 {

typedef unsigned char ko_t;      // a layer number 1 .. nk <= 128
constexpr int ND_BATCH = 4;      // tracers a flux kernel takes at a time: the surfaces are read once for all of them

// The surfaces of the faces, and what the flux kernels leave for the update kernels (nd_update_sym_kernel / nd_update_kernel)
struct NDFaces {
  GridDev g;
  const double *h;
  double scale;                      // I_numitts
  int ns;                            // surfaces of a face: 2nk+2 (continuous) or 4nk
  const double *khdt[2];
  double *PoL[2], *PoR[2], *hEff[2]; // [surface][faces of the direction]
  double *Flx[2];                    // (the order of 2024 and before) [surface][faces], + flx_stride per tracer of the batch
  double *tend[2][2];                // (the symmetric order) [direction][side of the face: the cell it is the E | N face of, the W | S face of]
                                     // [layer][faces]: the tendency of the cell's layer from this face, + flx_stride per tracer
  ko_t *KoL[2], *KoR[2];             // the reference's 1-based layer numbers
  int nb;                            // tracers in this batch (<= ND_BATCH)
  double *t[ND_BATCH];               // the tracers being diffused
  double cu[ND_BATCH];               // their conc_underflow
  long flx_stride;
  int *bad;                          // a word of bits the kernels raise; the branch's table says what each means
};

// What the diagnostic forms of the kernels take beside their arguments (the forms without diagnostics take nothing: they are the code they
// were).  NDTransOut: the flux kernels of the symmetric order, which never store the fluxes, keep one more sum per tracer of the batch --
// trans = trans - Coef(:,:,1)*Flx(ks), the value the tendencies get -- and store trans*Idt to a plane (dfx_2d / dfy_2d; null: this
// tracer did not ask).  NDMixOut: the update kernels store (dTracer(k)*IareaT)*Idt where dfxy_cont goes (the array, or scratch when only
// dfxy_cont_2d is asked for) and that value / (h + H_subroundoff) to dfxy_conc, and 0 on land.
struct NDTransOut { double *trans[ND_BATCH]; double Idt; };
struct NDMixOut { double *cont[ND_BATCH], *conc[ND_BATCH]; double Idt; };
template <typename T> __device__ __forceinline__ const T &nd_first(const T &t) { return t; }      // the one member of a kernel's pack

// The lane's face of the direction DIR (u faces I = isc-1 .. iec, j = jsc .. jec; v faces i = isc .. iec, J = jsc-1 .. jec) in a grid of
// nbx * rows blocks of 64 lanes: its plane offset f and plane size pl, the columns cl, cr on its two sides; has: the lane has a face
struct NDFace { int i, j; long f, pl, hpl, cl, cr; bool has, wet; };
template <int DIR>
__device__ __forceinline__ NDFace nd_face(const GridDev &g, int nbx) {
  NDFace F;
  const int bx = blockIdx.x % nbx, by = blockIdx.x / nbx;
  F.i = (DIR ? g.isc : g.isc - 1) + bx * 64 + threadIdx.x; F.j = (DIR ? g.jsc - 1 : g.jsc) + by;
  F.has = F.i <= g.iec;
  F.f = DIR ? g.v2(F.i, F.j) : g.u2(F.i, F.j); F.pl = DIR ? (long)g.nih * (g.njh + 1) : (long)(g.nih + 1) * g.njh;
  F.hpl = (long)g.nih * g.njh; F.cl = g.h2(F.i, F.j); F.cr = DIR ? g.h2(F.i, F.j + 1) : g.h2(F.i + 1, F.j);
  F.wet = F.has && (DIR ? g.mask2dCv[F.f] : g.mask2dCu[F.f]) > 0.0;
  return F;
}
// The lane's h column of the compute domain with a halo of 1
struct NDCol { int i, j; long n2, hpl; bool has; };
__device__ __forceinline__ NDCol nd_column(const GridDev &g, int nbx) {
  NDCol C;
  const int bx = blockIdx.x % nbx, by = blockIdx.x / nbx;
  C.i = g.isc - 1 + bx * 64 + threadIdx.x; C.j = g.jsc - 1 + by;
  C.has = C.i <= g.iec + 1;
  C.n2 = g.h2(C.i, C.j); C.hpl = (long)g.nih * g.njh;
  return C;
}

// boundary_k_range(SURFACE, ...), src/tracer/MOM_hor_bnd_diffusion.F90:609-647, for a column of nk thicknesses `stride` apart: k_bot
// (1-based) and zeta_bot
__device__ __forceinline__ void boundary_k_range_surface(const double *__restrict__ h, long stride, int nk, double hbl, int &k_bot,
                                                         double &zeta_bot) {
  k_bot = 1; zeta_bot = 0.;
  if (hbl == 0.) return;
  double hsum = 0., htot = 0.;
  for (int k = 0; k < nk; k++) hsum = hsum + h[stride * k];
  if (hbl >= hsum) { k_bot = nk; zeta_bot = 1.; return; }
  for (int k = 0; k < nk; k++) {
    const double hk = h[stride * k];
    htot = htot + hk;
    if (htot >= hbl) { k_bot = k + 1; zeta_bot = 1 - (htot - hbl) / hk; return; }
  }
}

// What the arrays hold where no surfaces are searched for (MOM_neutral_diffusion.F90:472-481, :510-519), and the fluxes or tendencies
// of a tracer there (f: with the tracer's offset in the batch, or the pointers with it)
template <int DIR>
__device__ __forceinline__ void nd_dry_surfaces(const NDFaces &S, long f, long pl) {
  for (int ks = 0; ks < S.ns; ks++) {
    S.PoL[DIR][f + pl * ks] = 0.; S.PoR[DIR][f + pl * ks] = 0.; S.KoL[DIR][f + pl * ks] = 1; S.KoR[DIR][f + pl * ks] = 1;
    if (ks < S.ns - 1) S.hEff[DIR][f + pl * ks] = 0.;
  }
}
template <bool SYM>
__device__ __forceinline__ void nd_dry_fluxes(int ns, int nk, double *__restrict__ Flx, double *__restrict__ tdL, double *__restrict__ tdR, long f, long pl) {
  if (SYM) for (int k = 0; k < nk; k++) { tdL[f + pl * k] = 0.; tdR[f + pl * k] = 0.; }
  else for (int ks = 0; ks < ns - 1; ks++) Flx[f + pl * ks] = 0.;
}

// The symmetric order: a surface never lies above the one before it, so the sum of a layer is a run of consecutive surfaces and is kept
// in a register.  The surface leaves the layer kt for the layer kb: the sum is stored and the layers between, which no sublayer lies
// in, get zeros.  kt = -1 is the head of the column (nothing to store), kb = nk its tail; every layer is stored once.
__device__ __forceinline__ void nd_tend_store(double *__restrict__ td, long f, long pl, int kt, int kb, double acc) {
  if (kt >= 0) td[f + pl * kt] = acc;
  for (int k = kt + 1; k < kb; k++) td[f + pl * k] = 0.;
}

// What a reconstruction supplies to neutral_drive.  The launches read the branch's kernel arguments, whose face state is the NDFaces
// the driver was given and fills.
struct NDBranch {
  int ns;
  std::function<int(const double *hbl)> scratch;      // its own scratch; hbl: CS%hbl with its halo (NDIFF_INTERIOR_ONLY) or null
  std::function<int()> surfaces;                      // neutral_diffusion_calc_coeffs :337 after the pass of CS%hbl
  std::function<int()> once;                          // (optional) what it forms once a call, after the first surfaces
  std::function<void()> tracer_cols;                  // the reconstructions of the batch's tracers
  // neutral_surface_flux of the batch: tendencies (symmetric) or fluxes; tx, ty: with the symmetric order, where dfx_2d / dfy_2d of the
  // batch go (null: none of the batch asked for the direction's -- the launch without diagnostics)
  std::function<void(bool symmetric, const NDTransOut *tx, const NDTransOut *ty)> fluxes;
  bool flux_has_coef;                                 // the fluxes carry the diffusivity (KHTR_USE_EBT_STRUCT, :834-848)
  struct Bad { int bit; const char *message; };
  std::vector<Bad> bad;                               // the bits of NDFaces::bad, in the order they are reported
};
// neutral_diffusion's outer structure (MOM_tracer_hor_diff.F90:474-534, MOM_neutral_diffusion.F90:605-960) for either reconstruction
// (neutral_diffusion.hip, beside the update kernels)
int neutral_drive(const HordiffCall &c, const mom6hip_neutral_diffusion_cs_t *nd, NDFaces &S, const NDBranch &b);

}  // namespace m6
