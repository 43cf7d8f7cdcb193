"""Host-side mirror of MOM_tracer_hor_diff (reference: src/tracer/MOM_tracer_hor_diff.F90): tracer_hor_diff_init (:1625) and
tracer_hordiff (:119) -- the along-layer diffusion with a constant KHTR or the VarMix / MEKE diffusivities of :236-281, and with
USE_NEUTRAL_DIFFUSION the continuous branch of MOM_neutral_diffusion (:474-534; mom6_amd/csrc/neutral_diffusion.hip), with
DIFFUSE_ML_TO_INTERIOR tracer_epipycnal_ML_diff (:700; mom6_amd/csrc/epipycnal_diff.hip), and with USE_HORIZONTAL_BOUNDARY_DIFFUSION the
horizontal boundary diffusion of src/tracer/MOM_hor_bnd_diffusion.F90 before either branch (:408-472; mom6_amd/csrc/hor_bnd_diffusion.hip).
With KHTR_USE_EBT_STRUCT the interface coefficients of the neutral and the boundary-diffusion branch decay with VarMix%ebt_struct
(:428-462, :503-518; FULL_DEPTH_KHTR_MIN), and with NDIFF_TAPERING the neutral fluxes are tapered across the transition zone.
The work is done by libmom6hip (mom6_amd/csrc/tracer_hor_diff.hip)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._lib import Mom6HipError, check, lib
from .tracer_advect import DeviceGrid, _ptr_space, flux_diag_records

_PARAMS = {"KHTR": "KhTr", "MAX_TR_DIFFUSION_CFL": "max_diff_CFL", "CHECK_DIFFUSIVE_CFL": "check_diffusive_CFL", "KHTR_SLOPE_CFF": "KhTr_Slope_Cff",
           "KHTR_MIN": "KhTr_min", "KHTR_MAX": "KhTr_max", "KHTR_PASSIVITY_COEFF": "KhTr_passivity_coeff", "KHTR_PASSIVITY_MIN": "KhTr_passivity_min"}
# hor_bnd_diffusion_init (src/tracer/MOM_hor_bnd_diffusion.F90:79-158): its parameters (module MOM_hor_bnd_diffusion) and their defaults
_HBD_PARAMS = {"HBD_LINEAR_TRANSITION": "linear", "APPLY_LIMITER": "limiter", "APPLY_LIMITER_REMAP": "limiter_remap",
               "HBD_BOUNDARY_EXTRAP": "boundary_extrap", "HBD_DEBUG": "debug"}
# DIFFUSE_ML_TO_INTERIOR and its parameters (:1687-1727)
_EPI_PARAMS = {"ML_KHTR_SCALE": ("ML_KhTr_scale", float), "HOR_DIFF_ANSWER_DATE": ("answer_date", int), "HOR_DIFF_LIMIT_BUG": ("limit_bug", bool)}
# neutral_diffusion_init (src/tracer/MOM_neutral_diffusion.F90:138): the parameters of the continuous branch, and those refused
_ND_PARAMS = {"NDIFF_REF_PRES": ("ref_pres", float), "NDIFF_ANSWER_DATE": ("ndiff_answer_date", int), "RECALC_NEUTRAL_SURF": ("recalc_neutral_surf", bool),
              "NDIFF_INTERIOR_ONLY": ("interior_only", bool)}
_ND_REFUSED = {"NDIFF_USE_UNMASKED_TRANSPORT_BUG": 4}
# the parameters neutral_diffusion_init reads with NDIFF_CONTINUOUS = False only (:219-277)
_NDD_PARAMS = {"NDIFF_BOUNDARY_EXTRAP": ("boundary_extrap", bool), "REMAPPING_ANSWER_DATE": ("remap_answer_date", int),
               "NEUTRAL_POS_METHOD": ("neutral_pos_method", int), "NDIFF_DRHO_TOL": ("drho_tol", float), "NDIFF_X_TOL": ("x_tol", float),
               "NDIFF_MAX_ITER": ("max_iter", int), "HARD_FAIL_HEFF": ("hard_fail_heff", bool)}


class tracer_hor_diff_CS:
    """tracer_hor_diff_CS (:40-100); parameters by their reference names (defaults :1652-1700).

    NDIFF_CONTINUOUS = False (the discontinuous reconstructions of MOM_neutral_diffusion) is taken only when NDIFF_REMAPPING_SCHEME is
    named with it (PLM, the reference's default, PPM_H4 or PPM_IH4); its other parameters (NDIFF_BOUNDARY_EXTRAP, REMAPPING_ANSWER_DATE,
    NEUTRAL_POS_METHOD, DELTA_RHO_FORM, NDIFF_DRHO_TOL, NDIFF_X_TOL, NDIFF_MAX_ITER, HARD_FAIL_HEFF, NDIFF_DEBUG) keep the reference's
    defaults.  NDIFF_CONTINUOUS = False alone goes on being refused at the call, by the library and with the words it has always used
    (the mirror adds that the scheme has to be named):
    tests/test_neutral_diffusion.py::test_tracer_hordiff_neutral_refuses_what_it_does_not_provide calls it so and expects the error, and
    that test stays as it is -- the arrangement that keeps its NDIFF_TAPERING line true."""

    def __init__(self, **params):
        st = self.st = _abi.TracerHorDiffCS()
        st.KhTr, st.max_diff_CFL, st.check_diffusive_CFL, st.KhTr_passivity_min = 0.0, -1.0, 0, 0.5
        nd = self.neutral_diffusion_CSp = _abi.NeutralDiffusionCS()
        nd.ref_pres, nd.ndiff_answer_date, nd.H_to_RZ = -1.0, 20240101, 0.0      # H_to_RZ: GV%H_to_RZ, taken from the grid at the call
        ep = self.epipycnal = _abi.EpipycnalCS()
        ep.ML_KhTr_scale, ep.answer_date, ep.limit_bug = 1.0, 20240101, 1
        hb = self.hor_bnd_diffusion_CSp = _abi.HorBndDiffusionCS()
        hb.limiter, hb.remap_scheme = 1, _abi.REMAP_SCHEMES["PLM"]
        ndd = self.ndiff_discontinuous = _abi.NdiffDiscontinuousCS()
        ndd.drho_tol, ndd.x_tol, ndd.remap_scheme, ndd.remap_answer_date = 1.0e-10, 0.0, _abi.REMAP_SCHEMES["PLM"], 99991231
        ndd.neutral_pos_method, ndd.delta_rho_form, ndd.max_iter, ndd.hard_fail_heff = 3, _abi.DELTA_RHO_FORMS["mid_pressure"], 10, 1
        self.discontinuous = False      # NDIFF_REMAPPING_SCHEME was named: the library gets ndiff_discontinuous
        full_depth = False
        for k, v in params.items():
            if k == "KHTR_USE_EBT_STRUCT":      # the one parameter both control structures read (:1655; MOM_neutral_diffusion.F90:199)
                st.unsupported[5] = nd.unsupported[3] = int(bool(v))
            elif k == "FULL_DEPTH_KHTR_MIN":
                full_depth = bool(v)
            elif k == "NDIFF_TAPERING":
                nd.unsupported[2] = int(bool(v))      # CS%tapering (taken by the neutral branch)
            elif k == "USE_HORIZONTAL_BOUNDARY_DIFFUSION":
                st.unsupported[1] = int(bool(v))      # CS%use_hor_bnd_diffusion (taken by mom6hip_tracer_hordiff_hbd)
            elif k in _HBD_PARAMS:
                setattr(hb, _HBD_PARAMS[k], int(bool(v)))
            elif k == "HBD_REMAPPING_SCHEME":
                if v not in _abi.HBD_REMAPPING_SCHEMES:
                    raise Mom6HipError(f"hor_bnd_diffusion: HBD_REMAPPING_SCHEME = {v} is not provided by libmom6hip "
                                       f"({', '.join(_abi.HBD_REMAPPING_SCHEMES)} are)")
                hb.remap_scheme = _abi.REMAP_SCHEMES[v]
            elif k == "DIFFUSE_ML_TO_INTERIOR":
                st.unsupported[2] = int(bool(v))      # CS%Diffuse_ML_interior (taken by mom6hip_tracer_hordiff_epipycnal)
            elif k in _EPI_PARAMS:
                setattr(ep, _EPI_PARAMS[k][0], _EPI_PARAMS[k][1](v))
            elif k == "USE_NEUTRAL_DIFFUSION":
                st.unsupported[0] = int(bool(v))      # CS%use_neutral_diffusion (taken by mom6hip_tracer_hordiff_neutral)
            elif k in _ND_PARAMS:
                setattr(nd, _ND_PARAMS[k][0], _ND_PARAMS[k][1](v))
            elif k == "NDIFF_CONTINUOUS":
                nd.unsupported[0] = int(not v)
            elif k == "NDIFF_REMAPPING_SCHEME":
                if v not in _abi.NDIFF_REMAPPING_SCHEMES:
                    raise Mom6HipError(f"neutral_diffusion: NDIFF_REMAPPING_SCHEME = {v} is not provided by libmom6hip "
                                       f"({', '.join(_abi.NDIFF_REMAPPING_SCHEMES)} are)")
                ndd.remap_scheme = _abi.REMAP_SCHEMES[v]; self.discontinuous = True
            elif k == "DELTA_RHO_FORM":
                if v not in _abi.DELTA_RHO_FORMS:
                    raise Mom6HipError(f"neutral_diffusion: DELTA_RHO_FORM = {v}: delta_rho_form is not recognized")
                ndd.delta_rho_form = _abi.DELTA_RHO_FORMS[v]
            elif k in _NDD_PARAMS:
                setattr(ndd, _NDD_PARAMS[k][0], int(_NDD_PARAMS[k][1](v)) if _NDD_PARAMS[k][1] is bool else _NDD_PARAMS[k][1](v))
            elif k == "NDIFF_DEBUG":
                pass      # only prints
            elif k in _ND_REFUSED:
                nd.unsupported[_ND_REFUSED[k]] = int(bool(v))
            elif k == "GV_H_to_RZ":
                nd.H_to_RZ = float(v)
            elif k in _PARAMS:
                a = _PARAMS[k]
                setattr(st, a, int(bool(v)) if a == "check_diffusive_CFL" else float(v))
            else:
                raise Mom6HipError(f"tracer_hor_diff_init: unknown parameter {k}")
        st.full_depth_khtr_min = int(full_depth and bool(st.unsupported[5]) and st.KhTr_min > 0.0)      # read only then (:1667)
        if nd.unsupported[2] and not nd.interior_only:      # the reference reads the parameter with NDIFF_INTERIOR_ONLY only
            raise Mom6HipError("neutral_diffusion: NDIFF_TAPERING is read with NDIFF_INTERIOR_ONLY only: it is refused without")
        if st.unsupported[0] and st.unsupported[2]:
            raise Mom6HipError("MOM_tracer_hor_diff: USE_NEUTRAL_DIFFUSION and DIFFUSE_ML_TO_INTERIOR are mutually exclusive!")      # :1732
        if st.unsupported[1] and st.unsupported[2]:
            raise Mom6HipError("MOM_tracer_hor_diff: USE_HORIZONTAL_BOUNDARY_DIFFUSION and DIFFUSE_ML_TO_INTERIOR are mutually exclusive!")      # :1735
        st.initialized = 1; nd.initialized = 1; hb.initialized = 1; ndd.initialized = 1
        self.last = None


def tracer_hor_diff_init(Time=None, G=None, GV=None, US=None, param_file=None, diag=None, EOS=None, diabatic_CSp=None, **params):
    """tracer_hor_diff_init(Time, G, GV, US, param_file, diag, EOS, diabatic_CSp, CS) -- :1625 (parameters as keywords)."""
    return tracer_hor_diff_CS(**params)


def tracer_hordiff(h, dt, MEKE, VarMix, visc, G: DeviceGrid, CS: tracer_hor_diff_CS, Reg, tv=None, do_online_flag=None, read_khdt_x=None,
                   read_khdt_y=None, conc_underflow=None, GV=None, diag=None, mix_diag=None):
    """tracer_hordiff(h, dt, MEKE, VarMix, visc, G, GV, US, CS, Reg, tv, do_online_flag, read_khdt_x, read_khdt_y) -- :119.
    Reg: the list of tracer arrays (Reg%Tr(m)%t), updated in place.  VarMix: None, or a dict (its presence is
    VarMix%use_variable_mixing) with any of L2u, L2v, SN_u, SN_v (read with KHTR_SLOPE_CFF > 0), Res_fn_h (its presence is
    VarMix%Resoln_scaled_KhTr), Rd_dx_h (KHTR_PASSIVITY_COEFF > 0); MEKE: None, or a dict with Kh (MEKE%Kh) and KhTr_fac
    (MEKE%KhTr_fac); MEKE%Kh is read with variable mixing only, as in the reference.  With KHTR_USE_EBT_STRUCT VarMix has ebt_struct
    (VarMix%ebt_struct: h points, nk levels, a valid halo of 1) too.  diag: None, or one entry per tracer, each None or a dict with
    any of df_x, df_y (u / v points, nk layers) and df2d_x, df2d_y (u / v points, a plane) -- Reg%Tr(m)%df_x ... where associated, arrays
    in the memory space of the fields: the along-layer branch zeroes and fills them as the reference does (:389-406, :576-591); the other
    branches refuse them.  mix_diag: None, or one entry per tracer, each None or a dict with any of what neutral_diffusion posts (dfx_2d,
    dfy_2d: u / v points, a plane; dfxy_cont, dfxy_conc: h points, nk layers; dfxy_cont_2d: h points, a plane -- with USE_NEUTRAL_DIFFUSION)
    and of what hor_bnd_diffusion posts (hbd_dfx, hbd_dfy, hbd_dfx_2d, hbd_dfy_2d, hbdxy_cont, hbdxy_cont_2d, hbdxy_conc -- with
    USE_HORIZONTAL_BOUNDARY_DIFFUSION): arrays in the memory space of the fields, of which the call writes the compute range and nothing
    else (mom6hip_tracer_hordiff_mix_diag); with more than one iteration they are refused.  diag and mix_diag are independent of each
    other.  Returns the iteration statistics."""
    if CS is None or Reg is None:
        raise Mom6HipError("MOM_tracer_hor_diff: register_tracer must be called before tracer_hordiff.")
    if do_online_flag is False or read_khdt_x is not None or read_khdt_y is not None:
        raise Mom6HipError("tracer_hordiff (HIP): offline khdt arrays are not supported on this path")
    if diag is not None and not any(a is not None for d in diag for a in (d or {}).values()):
        diag = None
    if diag is not None and len(diag) != len(list(Reg)):
        raise Mom6HipError("tracer_hordiff: diag must have one entry per tracer")
    if diag is not None and CS.st.unsupported[0]:
        # USE_NEUTRAL_DIFFUSION: the along-layer loop does not run, and the reference leaves the arrays as :389-406 zeroed them
        if CS.st.KhTr > 0.0 or VarMix is not None:      # (:197 returns before anything is zeroed)
            _zero_flux_diag(G.grid, diag)
        diag = None
    if diag is not None and CS.st.unsupported[1]:
        # with USE_HORIZONTAL_BOUNDARY_DIFFUSION alone the reference runs the along-layer loop after the boundary diffusion (:536)
        raise Mom6HipError("tracer_hordiff (HIP): the diffusive flux diagnostics (df_x, df_y, df2d_x, df2d_y) together with "
                           "USE_HORIZONTAL_BOUNDARY_DIFFUSION and the along-layer diffusion are not provided by libmom6hip")
    if mix_diag is not None and not any(a is not None for d in mix_diag for a in (d or {}).values()):
        mix_diag = None
    if mix_diag is not None:
        if len(mix_diag) != len(list(Reg)):
            raise Mom6HipError("tracer_hordiff: mix_diag must have one entry per tracer")
        if not (CS.st.unsupported[0] or CS.st.unsupported[1]):
            raise Mom6HipError("tracer_hordiff: mix_diag holds the diagnostics of neutral_diffusion and hor_bnd_diffusion: it is refused without "
                               "USE_NEUTRAL_DIFFUSION or USE_HORIZONTAL_BOUNDARY_DIFFUSION")
        return _tracer_hordiff_mix(h, dt, MEKE, VarMix, visc, G, CS, Reg, tv, conc_underflow, mix_diag)
    if CS.st.unsupported[0] and CS.neutral_diffusion_CSp.unsupported[0]:
        return _tracer_hordiff_neutral_discontinuous(h, dt, MEKE, VarMix, visc, G, CS, Reg, tv, conc_underflow)
    if CS.st.unsupported[1]:
        return _tracer_hordiff_hbd(h, dt, MEKE, VarMix, visc, G, CS, Reg, tv, conc_underflow)
    if CS.st.unsupported[0]:
        return _tracer_hordiff_neutral(h, dt, MEKE, VarMix, visc, G, CS, Reg, tv, conc_underflow)
    if CS.st.unsupported[2]:
        return _tracer_hordiff_epipycnal(h, dt, MEKE, VarMix, G, GV, CS, Reg, tv, conc_underflow, diag)
    L = lib()
    entry = L.mom6hip_tracer_hordiff_varmix if diag is None else L.mom6hip_tracer_hordiff_diag      # (without diagnostics: the entry as ever)
    entry.argtypes = [C.c_void_p, C.POINTER(_abi.TracerHorDiffCS), C.POINTER(_abi.HorDiffFields), C.c_void_p, C.c_double,
                      C.POINTER(C.c_void_p), C.c_void_p, C.c_int32, C.c_int32, C.POINTER(_abi.HorDiffStats)] + ([] if diag is None else [C.c_void_p])
    tr = list(Reg)
    spaces = set()
    hp, s0 = _ptr_space(h); spaces.add(s0)
    F = _abi.HorDiffFields()
    st = CS.st
    st.use_variable_mixing = int(VarMix is not None)
    st.Resoln_scaled_KhTr = int(VarMix is not None and VarMix.get("Res_fn_h") is not None)
    _check_VarMix(VarMix, CS)
    for n, a in list((VarMix or {}).items()) + ([("MEKE_Kh", MEKE.get("Kh"))] if MEKE else []):
        if a is not None:
            p, s = _ptr_space(a); spaces.add(s); setattr(F, n, p)
    if MEKE:
        st.KhTr_fac = float(MEKE.get("KhTr_fac", 1.0))
    ptrs = (C.c_void_p * max(len(tr), 1))()
    for m, t in enumerate(tr):
        p, s = _ptr_space(t); ptrs[m] = p; spaces.add(s)
    dg = _diff_diag_records(G.grid, diag, spaces)
    if len(spaces) != 1:
        raise Mom6HipError("tracer_hordiff: h, every tracer and every flux diagnostic must be in the same memory space")
    cu = None if conc_underflow is None else np.ascontiguousarray(conc_underflow, dtype=np.float64)
    stats = _abi.HorDiffStats()
    check(entry(G.handle, C.byref(CS.st), C.byref(F), C.c_void_p(hp), float(dt), ptrs, None if cu is None else cu.ctypes.data,
                len(tr), spaces.pop(), C.byref(stats), *(() if dg is None else (dg,))), "tracer_hordiff")
    CS.last = stats
    return stats


def _diff_diag_records(g, diag, spaces):
    """the records of the diffusive flux diagnostics of a call (None: none asked for); their memory spaces join `spaces`"""
    if diag is None:
        return None
    shapes = dict(df_x=g.shape3(_abi.POS_U), df_y=g.shape3(_abi.POS_V), df2d_x=g.shape2(_abi.POS_U), df2d_y=g.shape2(_abi.POS_V))

    def P(a, kind, name):
        if tuple(a.shape) != shapes[kind]:
            raise Mom6HipError(f"tracer_hordiff: {name} has shape {tuple(a.shape)}, expected {shapes[kind]}")
        p, s = _ptr_space(a); spaces.add(s)
        return p
    return flux_diag_records(diag, _abi.DIFF_DIAGS, {n: n for n in _abi.DIFF_DIAGS}, P, "tracer_hordiff")


def _zero_flux_diag(g, diag):
    """:389-406: the arrays asked for are set to zero over I = is-1..ie, j = js..je and J = js-1..je, i = is..ie"""
    for d in diag:
        for n, a in (d or {}).items():
            if n not in _abi.DIFF_DIAGS:
                raise Mom6HipError(f"tracer_hordiff: {n} is not a flux diagnostic of this operator ({', '.join(_abi.DIFF_DIAGS)} are)")
            if a is not None:
                sj, si = g.csl(_abi.POS_U if n.endswith("x") else _abi.POS_V)
                a[..., sj, si] = 0.0


def _check_VarMix(VarMix, CS):
    """the fields of VarMix this path reads: ebt_struct with KHTR_USE_EBT_STRUCT only, and then it must be there where it is read"""
    ebt = bool(CS.st.unsupported[5])
    allowed = set(_abi.HORDIFF_FIELDS) | ({_abi.HORDIFF_EBT_FIELD} if ebt else set())
    if set(VarMix or {}) - allowed:
        raise Mom6HipError("tracer_hordiff (HIP): of VarMix only L2u/v, SN_u/v, Res_fn_h and Rd_dx_h are read"
                           + (" (and ebt_struct with KHTR_USE_EBT_STRUCT)" if not ebt else ", and ebt_struct"))
    if ebt and (CS.st.unsupported[0] or CS.st.unsupported[1]) and (VarMix or {}).get(_abi.HORDIFF_EBT_FIELD) is None:
        raise Mom6HipError("tracer_hordiff: KHTR_USE_EBT_STRUCT needs VarMix%ebt_struct")


def _same(a, b):
    return a is b or (hasattr(a, "data_ptr") and hasattr(b, "data_ptr") and a.data_ptr() == b.data_ptr())


def _tv_TS(tv, tr, what):
    """(get, [idx_T, idx_S]): tv%T and tv%S among the registered tracers (the reference's registry points at them)"""
    get = (lambda n: tv.get(n)) if isinstance(tv, dict) else (lambda n: getattr(tv, n, None))
    if tv is None or get("T") is None or get("S") is None or get("eqn_of_state") is None:
        raise Mom6HipError(f"tracer_hordiff: {what} needs tv%T, tv%S and tv%eqn_of_state")
    idx = [next((m for m, t in enumerate(tr) if _same(t, get(n))), -1) for n in ("T", "S")]
    if min(idx) < 0:
        raise Mom6HipError("tracer_hordiff: tv%T and tv%S must be registered tracers (entries of Reg)")
    return get, idx


def _marshal(h, MEKE, VarMix, CS, tr):
    """the arguments every entry point takes: (h pointer, the MEKE / VarMix fields, the tracer table, the memory spaces seen so far)"""
    _check_VarMix(VarMix, CS)
    spaces = set()
    hp, s0 = _ptr_space(h); spaces.add(s0)
    F = _abi.HorDiffFields()
    st = CS.st
    st.use_variable_mixing = int(VarMix is not None)
    st.Resoln_scaled_KhTr = int(VarMix is not None and VarMix.get("Res_fn_h") is not None)
    for n, a in list((VarMix or {}).items()) + ([("MEKE_Kh", MEKE.get("Kh"))] if MEKE else []):
        if a is not None:
            p, s = _ptr_space(a); spaces.add(s); setattr(F, n, p)
    if MEKE:
        st.KhTr_fac = float(MEKE.get("KhTr_fac", 1.0))
    ptrs = (C.c_void_p * max(len(tr), 1))()
    for m, t in enumerate(tr):
        p, s = _ptr_space(t); ptrs[m] = p; spaces.add(s)
    return hp, F, ptrs, spaces


def _h_ML(visc):
    hml = None if visc is None else (visc.get("h_ML") if isinstance(visc, dict) else getattr(visc, "h_ML", None))
    if hml is None:
        raise Mom6HipError("hor_bnd_diffusion requires that visc%h_ML is associated.")
    return hml


def _tracer_hordiff_neutral(h, dt, MEKE, VarMix, visc, G, CS, Reg, tv, conc_underflow):
    """the USE_NEUTRAL_DIFFUSION branch (:474-534): tv has T, S (two of the arrays of Reg, as in the reference where the registry
    points at tv%T and tv%S), eqn_of_state (an _abi.EOS) and optionally p_surf -- a dict or an object; with NDIFF_INTERIOR_ONLY visc
    has h_ML (visc%h_ML, the boundary-layer depth)."""
    tr = list(Reg)
    get, idx = _tv_TS(tv, tr, "USE_NEUTRAL_DIFFUSION")
    L = lib()
    L.mom6hip_tracer_hordiff_neutral.argtypes = [C.c_void_p, C.POINTER(_abi.TracerHorDiffCS), C.POINTER(_abi.NeutralDiffusionCS),
                                                 C.POINTER(_abi.HorDiffFields), C.c_void_p, C.POINTER(_abi.EOS), C.c_void_p, C.c_double,
                                                 C.POINTER(C.c_void_p), C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                 C.POINTER(_abi.HorDiffStats)]
    hp, F, ptrs, spaces = _marshal(h, MEKE, VarMix, CS, tr)
    st = CS.st
    if CS.neutral_diffusion_CSp.interior_only:
        p, s = _ptr_space(_h_ML(visc)); spaces.add(s); F.h_ML = p
    ps = None
    if get("p_surf") is not None:
        ps, s = _ptr_space(get("p_surf")); spaces.add(s)
    if len(spaces) != 1:
        raise Mom6HipError("tracer_hordiff: h, p_surf and every tracer must be in the same memory space")
    nd = CS.neutral_diffusion_CSp
    if nd.H_to_RZ == 0.0:
        nd.H_to_RZ = float(G.grid.Rho0 * G.grid.H_to_Z)      # GV%H_to_RZ, Boussinesq
    cu = None if conc_underflow is None else np.ascontiguousarray(conc_underflow, dtype=np.float64)
    stats = _abi.HorDiffStats()
    check(L.mom6hip_tracer_hordiff_neutral(G.handle, C.byref(st), C.byref(nd), C.byref(F), C.c_void_p(hp), C.byref(get("eqn_of_state")),
                                           None if ps is None else C.c_void_p(ps), float(dt), ptrs, None if cu is None else cu.ctypes.data,
                                           len(tr), idx[0], idx[1], spaces.pop(), C.byref(stats)), "tracer_hordiff")
    CS.last = stats
    return stats


def _tracer_hordiff_hbd(h, dt, MEKE, VarMix, visc, G, CS, Reg, tv, conc_underflow):
    """USE_HORIZONTAL_BOUNDARY_DIFFUSION (:408-472) and then the neutral branch (USE_NEUTRAL_DIFFUSION, tv as _tracer_hordiff_neutral takes
    it) or the along-layer diffusion: visc -- a dict or an object -- has h_ML (visc%h_ML, the boundary-layer depth)."""
    hml = _h_ML(visc)
    tr = list(Reg)
    st = CS.st
    neutral = bool(st.unsupported[0])
    idx, eos, p_surf = [0, 0], None, None
    if neutral:
        get, idx = _tv_TS(tv, tr, "USE_NEUTRAL_DIFFUSION")
        eos, p_surf = get("eqn_of_state"), get("p_surf")
    L = lib()
    L.mom6hip_tracer_hordiff_hbd.argtypes = [C.c_void_p, C.POINTER(_abi.TracerHorDiffCS), C.POINTER(_abi.HorBndDiffusionCS),
                                             C.POINTER(_abi.NeutralDiffusionCS), C.POINTER(_abi.HorDiffFields), C.c_void_p, C.POINTER(_abi.EOS),
                                             C.c_void_p, C.c_double, C.POINTER(C.c_void_p), C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_int32, C.POINTER(_abi.HorDiffStats)]
    hp, F, ptrs, spaces = _marshal(h, MEKE, VarMix, CS, tr)
    p, s = _ptr_space(hml); spaces.add(s); F.h_ML = p
    ps = None
    if p_surf is not None:
        ps, s = _ptr_space(p_surf); spaces.add(s)
    if len(spaces) != 1:
        raise Mom6HipError("tracer_hordiff: h, visc%h_ML, p_surf and every tracer must be in the same memory space")
    nd = CS.neutral_diffusion_CSp
    if neutral and nd.H_to_RZ == 0.0:
        nd.H_to_RZ = float(G.grid.Rho0 * G.grid.H_to_Z)      # GV%H_to_RZ, Boussinesq
    cu = None if conc_underflow is None else np.ascontiguousarray(conc_underflow, dtype=np.float64)
    stats = _abi.HorDiffStats()
    check(L.mom6hip_tracer_hordiff_hbd(G.handle, C.byref(st), C.byref(CS.hor_bnd_diffusion_CSp), C.byref(nd) if neutral else None, C.byref(F),
                                       C.c_void_p(hp), C.byref(eos) if neutral else None, None if ps is None else C.c_void_p(ps), float(dt),
                                       ptrs, None if cu is None else cu.ctypes.data, len(tr), idx[0], idx[1], spaces.pop(), C.byref(stats)),
          "tracer_hordiff")
    CS.last = stats
    return stats


def _tracer_hordiff_neutral_discontinuous(h, dt, MEKE, VarMix, visc, G, CS, Reg, tv, conc_underflow):
    """USE_NEUTRAL_DIFFUSION with NDIFF_CONTINUOUS = False (after USE_HORIZONTAL_BOUNDARY_DIFFUSION, if that is set): tv and visc as
    _tracer_hordiff_neutral and _tracer_hordiff_hbd take them.  The parameters of the branch go with the call only where
    NDIFF_REMAPPING_SCHEME was named (the class docstring says why); without them the library refuses NDIFF_CONTINUOUS = False."""
    tr = list(Reg)
    st, nd = CS.st, CS.neutral_diffusion_CSp
    hbd = bool(st.unsupported[1])
    get, idx = _tv_TS(tv, tr, "USE_NEUTRAL_DIFFUSION")
    L = lib()
    L.mom6hip_tracer_hordiff_neutral_discontinuous.argtypes = [
        C.c_void_p, C.POINTER(_abi.TracerHorDiffCS), C.POINTER(_abi.HorBndDiffusionCS), C.POINTER(_abi.NeutralDiffusionCS),
        C.POINTER(_abi.NdiffDiscontinuousCS), C.POINTER(_abi.HorDiffFields), C.c_void_p, C.POINTER(_abi.EOS), C.c_void_p, C.c_double,
        C.POINTER(C.c_void_p), C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_abi.HorDiffStats)]
    hp, F, ptrs, spaces = _marshal(h, MEKE, VarMix, CS, tr)
    if hbd or nd.interior_only:
        p, s = _ptr_space(_h_ML(visc)); spaces.add(s); F.h_ML = p
    ps = None
    if get("p_surf") is not None:
        ps, s = _ptr_space(get("p_surf")); spaces.add(s)
    if len(spaces) != 1:
        raise Mom6HipError("tracer_hordiff: h, visc%h_ML, p_surf and every tracer must be in the same memory space")
    if nd.H_to_RZ == 0.0:
        nd.H_to_RZ = float(G.grid.Rho0 * G.grid.H_to_Z)      # GV%H_to_RZ, Boussinesq
    cu = None if conc_underflow is None else np.ascontiguousarray(conc_underflow, dtype=np.float64)
    stats = _abi.HorDiffStats()
    try:
        check(L.mom6hip_tracer_hordiff_neutral_discontinuous(
            G.handle, C.byref(st), C.byref(CS.hor_bnd_diffusion_CSp) if hbd else None, C.byref(nd),
            C.byref(CS.ndiff_discontinuous) if CS.discontinuous else None, C.byref(F), C.c_void_p(hp), C.byref(get("eqn_of_state")),
            None if ps is None else C.c_void_p(ps), float(dt), ptrs, None if cu is None else cu.ctypes.data, len(tr), idx[0], idx[1],
            spaces.pop(), C.byref(stats)), "tracer_hordiff")
    except Mom6HipError as e:
        if CS.discontinuous or "NDIFF_CONTINUOUS" not in str(e):
            raise
        raise Mom6HipError(f"{e} (NDIFF_REMAPPING_SCHEME -- {', '.join(_abi.NDIFF_REMAPPING_SCHEMES)} -- has to be named with it)") from None
    CS.last = stats
    return stats


def _tracer_hordiff_mix(h, dt, MEKE, VarMix, visc, G, CS, Reg, tv, conc_underflow, mix_diag):
    """any pairing of USE_HORIZONTAL_BOUNDARY_DIFFUSION and USE_NEUTRAL_DIFFUSION (either reconstruction) with the diagnostics the two
    modules post themselves (mom6hip_tracer_hordiff_mix_diag); tv and visc as the branches take them"""
    tr = list(Reg)
    st, nd = CS.st, CS.neutral_diffusion_CSp
    hbd, neutral = bool(st.unsupported[1]), bool(st.unsupported[0])
    idx, eos, p_surf = [0, 0], None, None
    if neutral:
        get, idx = _tv_TS(tv, tr, "USE_NEUTRAL_DIFFUSION")
        eos, p_surf = get("eqn_of_state"), get("p_surf")
    L = lib()
    L.mom6hip_tracer_hordiff_mix_diag.argtypes = [
        C.c_void_p, C.POINTER(_abi.TracerHorDiffCS), C.POINTER(_abi.HorBndDiffusionCS), C.POINTER(_abi.NeutralDiffusionCS),
        C.POINTER(_abi.NdiffDiscontinuousCS), C.POINTER(_abi.HorDiffFields), C.c_void_p, C.POINTER(_abi.EOS), C.c_void_p, C.c_double,
        C.POINTER(C.c_void_p), C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_abi.HorDiffStats), C.c_void_p]
    hp, F, ptrs, spaces = _marshal(h, MEKE, VarMix, CS, tr)
    if hbd or (neutral and nd.interior_only):
        p, s = _ptr_space(_h_ML(visc)); spaces.add(s); F.h_ML = p
    ps = None
    if p_surf is not None:
        ps, s = _ptr_space(p_surf); spaces.add(s)
    g = G.grid
    recs = (_abi.TracerMixDiag * len(tr))()
    names = _abi.ND_MIX_DIAGS + _abi.HBD_MIX_DIAGS
    for m, d in enumerate(mix_diag):
        for n, a in (d or {}).items():
            if n not in names:
                raise Mom6HipError(f"tracer_hordiff: {n} is not a diagnostic of neutral_diffusion or hor_bnd_diffusion ({', '.join(names)} are)")
            if a is None:
                continue
            pos, rank = _abi.MIX_DIAG_KINDS[n]
            want = g.shape2(pos) if rank == 2 else g.shape3(pos)
            if tuple(a.shape) != want:
                raise Mom6HipError(f"tracer_hordiff: {n} of tracer {m + 1} has shape {tuple(a.shape)}, expected {want}")
            p, s = _ptr_space(a); spaces.add(s); setattr(recs[m], n, p)
    if len(spaces) != 1:
        raise Mom6HipError("tracer_hordiff: h, visc%h_ML, p_surf, every tracer and every diagnostic must be in the same memory space")
    if neutral and nd.H_to_RZ == 0.0:
        nd.H_to_RZ = float(G.grid.Rho0 * G.grid.H_to_Z)      # GV%H_to_RZ, Boussinesq
    cu = None if conc_underflow is None else np.ascontiguousarray(conc_underflow, dtype=np.float64)
    stats = _abi.HorDiffStats()
    check(L.mom6hip_tracer_hordiff_mix_diag(
        G.handle, C.byref(st), C.byref(CS.hor_bnd_diffusion_CSp) if hbd else None, C.byref(nd) if neutral else None,
        C.byref(CS.ndiff_discontinuous) if (neutral and CS.discontinuous) else None, C.byref(F), C.c_void_p(hp),
        C.byref(eos) if neutral else None, None if ps is None else C.c_void_p(ps), float(dt), ptrs, None if cu is None else cu.ctypes.data,
        len(tr), idx[0], idx[1], spaces.pop(), C.byref(stats), recs), "tracer_hordiff")
    CS.last = stats
    return stats


def _tracer_hordiff_epipycnal(h, dt, MEKE, VarMix, G, GV, CS, Reg, tv, conc_underflow, diag=None):
    """the DIFFUSE_ML_TO_INTERIOR branches (:544-550, :613-620 and tracer_epipycnal_ML_diff :700): tv has T, S (two of the arrays of
    Reg), eqn_of_state (an _abi.EOS) and P_Ref; GV -- a dict or an object -- has Rlay (nk values), nkml and nk_rho_varies."""
    get = (lambda n: tv.get(n)) if isinstance(tv, dict) else (lambda n: getattr(tv, n, None))
    gv = (lambda n: GV.get(n)) if isinstance(GV, dict) else (lambda n: getattr(GV, n, None))
    if tv is None or get("T") is None or get("S") is None or get("eqn_of_state") is None or get("P_Ref") is None:
        raise Mom6HipError("tracer_hordiff: DIFFUSE_ML_TO_INTERIOR needs tv%T, tv%S, tv%eqn_of_state and tv%P_Ref")
    if GV is None or gv("Rlay") is None or gv("nkml") is None or gv("nk_rho_varies") is None:
        raise Mom6HipError("tracer_hordiff: DIFFUSE_ML_TO_INTERIOR needs GV%Rlay, GV%nkml and GV%nk_rho_varies")
    tr = list(Reg)
    idx = [next((m for m, t in enumerate(tr) if _same(t, get(n))), -1) for n in ("T", "S")]
    if min(idx) < 0:
        raise Mom6HipError("tracer_hordiff: tv%T and tv%S must be registered tracers (entries of Reg)")
    _check_VarMix(VarMix, CS)
    L = lib()
    entry = L.mom6hip_tracer_hordiff_epipycnal if diag is None else L.mom6hip_tracer_hordiff_epipycnal_diag
    entry.argtypes = [C.c_void_p, C.POINTER(_abi.TracerHorDiffCS), C.POINTER(_abi.EpipycnalCS), C.POINTER(_abi.HorDiffFields), C.c_void_p,
                      C.POINTER(_abi.EOS), C.c_double, C.POINTER(C.c_void_p), C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                      C.POINTER(_abi.HorDiffStats)] + ([] if diag is None else [C.c_void_p])
    spaces = set()
    hp, s0 = _ptr_space(h); spaces.add(s0)
    F = _abi.HorDiffFields()
    st = CS.st
    st.use_variable_mixing = int(VarMix is not None)
    st.Resoln_scaled_KhTr = int(VarMix is not None and VarMix.get("Res_fn_h") is not None)
    for n, a in list((VarMix or {}).items()) + ([("MEKE_Kh", MEKE.get("Kh"))] if MEKE else []):
        if a is not None:
            p, s = _ptr_space(a); spaces.add(s); setattr(F, n, p)
    if MEKE:
        st.KhTr_fac = float(MEKE.get("KhTr_fac", 1.0))
    ptrs = (C.c_void_p * max(len(tr), 1))()
    for m, t in enumerate(tr):
        p, s = _ptr_space(t); ptrs[m] = p; spaces.add(s)
    dg = _diff_diag_records(G.grid, diag, spaces)
    if len(spaces) != 1:
        raise Mom6HipError("tracer_hordiff: h and every tracer must be in the same memory space")
    ep = CS.epipycnal
    Rlay = np.ascontiguousarray(gv("Rlay"), dtype=np.float64)
    if Rlay.size != G.grid.nk:
        raise Mom6HipError("tracer_hordiff: GV%Rlay must have nk values")
    ep.Rlay = Rlay.ctypes.data; ep.nkml, ep.nk_rho_varies, ep.P_Ref = int(gv("nkml")), int(gv("nk_rho_varies")), float(get("P_Ref"))
    cu = None if conc_underflow is None else np.ascontiguousarray(conc_underflow, dtype=np.float64)
    stats = _abi.HorDiffStats()
    check(entry(G.handle, C.byref(st), C.byref(ep), C.byref(F), C.c_void_p(hp), C.byref(get("eqn_of_state")), float(dt), ptrs,
                None if cu is None else cu.ctypes.data, len(tr), idx[0], idx[1], spaces.pop(), C.byref(stats), *(() if dg is None else (dg,))),
          "tracer_hordiff")
    CS.last = stats
    return stats
