"""The cases of the diagnostics neutral_diffusion and hor_bnd_diffusion post, shared by the CPU tests of the checker
(tests/test_tracer_mix_diag_checker.py) and the GPU tests of the library (tests/test_tracer_mix_diag.py): the shapes, the inputs, and the
checker's expectation of a case, formed once and left unchanged."""
import functools

import numpy as np

import hbd_checker as hc
import tracer_mix_checker as mc
from mom6_amd import _abi
from oracle import orc

DT, NTR, PAD, FILL, ZONE = 3600.0, 5, 257, 7.0, -12345.0
CU = [0.0, 0.0, 0.0, 0.05, 0.0]
SHAPES = {"20x5x3": dict(ni=20, nj=5, nk=3), "64x6x6": dict(ni=64, nj=6, nk=6), "70x9x3": dict(ni=70, nj=9, nk=3, reentrant=(False, False))}
PLM, H4 = dict(NDIFF_REMAPPING_SCHEME="PLM"), dict(NDIFF_REMAPPING_SCHEME="PPM_H4")
# name -> (shape, what the checker and the library are told).  taper / both need NDIFF_INTERIOR_ONLY, which the boundary-layer depth sets
CASES = {
    # (a) neutral diffusion on the continuous reconstruction
    "nd_20240101_plain": ("20x5x3", dict(date=20240101)), "nd_20240401_plain": ("64x6x6", dict(date=20240401)),
    "nd_20240101_taper": ("64x6x6", dict(date=20240101, taper=True)), "nd_20240401_taper": ("20x5x3", dict(date=20240401, taper=True)),
    "nd_20240101_ebt": ("70x9x3", dict(date=20240101, ebt=True, p_surf=True)), "nd_20240401_ebt": ("70x9x3", dict(date=20240401, ebt=True, p_surf=True)),
    "nd_20240101_both": ("20x5x3", dict(date=20240101, taper=True, ebt=True)), "nd_20240401_both": ("64x6x6", dict(date=20240401, taper=True, ebt=True)),
    # (b) NDIFF_CONTINUOUS = False
    "ndd_20240101_plm": ("20x5x3", dict(date=20240101, disc=PLM)), "ndd_20240401_plm": ("64x6x6", dict(date=20240401, disc=PLM)),
    "ndd_20240101_ppm_h4": ("64x6x6", dict(date=20240101, disc=H4)), "ndd_20240401_ppm_h4": ("20x5x3", dict(date=20240401, disc=H4)),
    # (c) boundary diffusion, then the along-layer loop
    "hbd_default": ("64x6x6", dict(hbd={}, neutral=False)), "hbd_linear": ("20x5x3", dict(hbd=dict(HBD_LINEAR_TRANSITION=True), neutral=False)),
    "hbd_limiter_remap": ("20x5x3", dict(hbd=dict(APPLY_LIMITER_REMAP=True), neutral=False)),
    "hbd_ebt_full_depth": ("70x9x3", dict(hbd={}, neutral=False, ebt=True, KhTr_min=2.0e3, full=True, dt=5.0)),
    # (d) boundary diffusion, then NDIFF_INTERIOR_ONLY neutral diffusion: all twelve
    "hbd_then_neutral": ("64x6x6", dict(hbd={}, date=20240401, interior=True)),
}


def names_of(kw):
    return (mc.HBD_NAMES if "hbd" in kw else ()) + (mc.ND_NAMES if kw.get("neutral", True) else ())


@functools.lru_cache(maxsize=None)
def state(shape):
    """grid, h, five tracers (T, S and three random ones), visc%h_ML, VarMix%ebt_struct, p_surf -- formed once a shape"""
    import test_hor_bnd_diffusion as thbd
    import test_ndiff_taper_ebt as tte
    g, h, tr, h_ML = thbd.case(ntr=2, hml=(0.1, 0.7), **SHAPES[shape])
    rng = np.random.default_rng(31)
    for _ in range(NTR - len(tr)):
        t = np.ascontiguousarray(rng.random(h.shape) * g.mask2dT[None])
        orc.halo_update(g, t, _abi.POS_H)
        tr.append(t)
    p_surf = np.ascontiguousarray(1.0e4 * np.random.default_rng(8).random(g.shape2(_abi.POS_H)))
    return g, h, tr, h_ML, tte.ebt_structure(g, decay=4.0), p_surf


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> g, the inputs, the checker's tracers, its arrays (FILL outside the compute range) for every tracer, its statistics, the library's
    parameters -- formed once a case and left unchanged"""
    shape, kw = CASES[name]
    g, h, tr0, h_ML, ebt_s, ps = state(shape)
    neutral, hbd, disc = kw.get("neutral", True), kw.get("hbd"), kw.get("disc")
    taper, ebt = kw.get("taper", False), kw.get("ebt", False)
    interior = bool(kw.get("interior", False) or taper)
    dt, KhTr_min, full, date = kw.get("dt", DT), kw.get("KhTr_min", 0.0), kw.get("full", False), kw.get("date", 20240101)
    KhTr = 5.0e3 if hbd is not None else 800.0
    use_hml = hbd is not None or interior
    tr = [t.copy() for t in tr0]
    mix = [{n: np.full(mc.shape_of(g, n), FILL) for n in names_of(kw)} for _ in range(NTR)]
    stats = mc.tracer_hordiff_mix(g, h, dt, tr, KhTr, orc.eos("WRIGHT"), hbd=None if hbd is None else hc.HBDCS(g.H_subroundoff, **hbd),
                                  neutral=neutral, disc=disc, h_ML=h_ML if use_hml else None, interior=interior,
                                  p_surf=ps if kw.get("p_surf") else None, ebt_struct=ebt_s if ebt else None, KhTr_min=KhTr_min,
                                  FULL_DEPTH_KHTR_MIN=full, conc_underflow=CU, mix=mix, NDIFF_ANSWER_DATE=date, NDIFF_TAPERING=taper)
    params = dict(KHTR=KhTr, KHTR_MIN=KhTr_min, FULL_DEPTH_KHTR_MIN=full, KHTR_USE_EBT_STRUCT=ebt)
    if hbd is not None:
        params.update(USE_HORIZONTAL_BOUNDARY_DIFFUSION=True, **hbd)
    if neutral:
        params.update(USE_NEUTRAL_DIFFUSION=True, NDIFF_ANSWER_DATE=date, NDIFF_INTERIOR_ONLY=interior, NDIFF_TAPERING=taper)
    if disc:
        params.update(NDIFF_CONTINUOUS=False, **disc)
    inputs = dict(h=h, tr=tr0, h_ML=h_ML if use_hml else None, ebt=ebt_s if ebt else None, p_surf=ps if kw.get("p_surf") else None, dt=dt,
                  neutral=neutral)
    return g, inputs, tr, mix, stats, params
