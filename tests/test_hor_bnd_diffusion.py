"""Horizontal boundary diffusion, USE_HORIZONTAL_BOUNDARY_DIFFUSION (src/tracer/MOM_hor_bnd_diffusion.F90; tracer_hordiff :408-472).
The checker (tests/hbd_checker.py) is pinned by every known answer of the reference's near_boundary_unit_tests (:831-1072,
tests/golden/hor_bnd_diffusion.json) and held to what the scheme guarantees; the library (mom6_amd/csrc/hor_bnd_diffusion.hip) is
compared with the checker followed by the unchanged orc.tracer_hordiff on the GPU, bit for bit."""
import functools
import json
import os
import socket
import subprocess

import numpy as np
import pytest

import hbd_checker as hc
from helpers import bits_equal, interior
from mom6_amd import _abi, synth
from oracle import orc

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "hor_bnd_diffusion.json")))


# ---- the reference's own unit-test answers ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", GOLD["boundary_k_range"], ids=[c["title"] for c in GOLD["boundary_k_range"]])
def test_boundary_k_range_known_answers(c):
    b = hc.SURFACE if c["boundary"] == "SURFACE" else hc.BOTTOM
    assert hc.boundary_k_range(b, len(c["h"]), c["h"], c["hbl"]) == (c["k_top"], c["zeta_top"], c["k_bot"], c["zeta_bot"])


@pytest.mark.parametrize("c", GOLD["sort_unique"], ids=[c["title"] for c in GOLD["sort_unique"]])
def test_sort_and_unique_known_answers(c):
    got = hc.sort(c["val"]) if c["op"] == "sort" else hc.unique(c["val"], c.get("val_max"))
    assert got[:c["n"]] == c["ans"]


@pytest.mark.parametrize("c", GOLD["merge_interfaces"], ids=[c["title"] for c in GOLD["merge_interfaces"]])
def test_merge_interfaces_known_answers(c):
    dz = hc.merge_interfaces(c["nk"], c["h_L"], c["h_R"], c["hbl_L"], c["hbl_R"], GOLD["settings"]["H_subroundoff"])
    assert dz[:c["n"]] == c["ans"]


@pytest.mark.parametrize("c", GOLD["fluxes_layer_method"], ids=[c["title"] for c in GOLD["fluxes_layer_method"]])
def test_fluxes_layer_method_known_answers(c):
    s = GOLD["settings"]
    CS = hc.HBDCS(s["H_subroundoff"], HBD_REMAPPING_SCHEME=s["HBD_REMAPPING_SCHEME"], HBD_BOUNDARY_EXTRAP=s["HBD_BOUNDARY_EXTRAP"],
                  HBD_LINEAR_TRANSITION=s["HBD_LINEAR_TRANSITION"], APPLY_LIMITER=s["APPLY_LIMITER"], APPLY_LIMITER_REMAP=s["APPLY_LIMITER_REMAP"])
    nk = len(c["h_L"])
    dz = hc.merge_interfaces(nk, c["h_L"], c["h_R"], c["hbl_L"], c["hbl_R"], CS.H_subroundoff)      # hbd_grid_test :1133
    F = hc.fluxes_layer_method(hc.SURFACE, nk, c["hbl_L"], c["hbl_R"], c["h_L"], c["h_R"], c["phi_L"], c["phi_R"], c["khtr_u"],
                               s["area_L"], s["area_R"], len(dz), dz, CS)
    assert F == c["F_layer"]


# ---- the 3-D scheme on the checker -------------------------------------------------------------------------------------------------
def case(ni=24, nj=16, nk=6, seed=5, reentrant=(True, False), land_frac=0.2, ntr=2, thin=True, hml=(0.0, 1.2)):
    """a grid with land, vanished layers and a boundary layer from none at all to deeper than the column"""
    g = synth.make_grid(ni, nj, nk, land_frac=land_frac, seed=seed + 900, reentrant_x=reentrant[0], reentrant_y=reentrant[1])
    d = {k: v.numpy() for k, v in synth.make_dynamics_state(g, seed=seed, umax=0.1, eta_amp=0.2).items()}
    rng = np.random.default_rng(seed)
    h = np.ascontiguousarray(d["h"])
    if thin:
        h = np.ascontiguousarray(h * np.where(rng.random(h.shape) < 0.1, 0.0, 1.0))
    T = np.ascontiguousarray(d["T"] + 0.5 * rng.standard_normal(h.shape)); S = np.ascontiguousarray(d["S"] + 0.05 * rng.standard_normal(h.shape))
    tr = [T, S, np.ascontiguousarray((rng.random(h.shape) > 0.7) * 1.0 * g.mask2dT[None])][:ntr]
    frac = np.clip(hml[0] + (hml[1] - hml[0]) * rng.random(g.shape2(_abi.POS_H)) - 0.1, 0.0, None)
    h_ML = np.ascontiguousarray(frac * h.sum(0))
    for t in tr + [h, h_ML]:
        orc.halo_update(g, t, _abi.POS_H)
    return g, h, tr, h_ML


def inventory(g, h, t):
    hh = interior(g, h) + g.H_subroundoff
    return float((hh * interior(g, g.areaT)[None] * interior(g, t)).sum())


def test_checker_conserves_and_keeps_constants():
    g, h, tr, h_ML = case()
    const = np.full_like(tr[0], -2.25)
    tr = [t.copy() for t in tr] + [const]
    before = [t.copy() for t in tr]
    CS = hc.HBDCS(g.H_subroundoff)
    n = hc.tracer_hordiff_hbd(g, h, 3600.0, tr, 5.0e3, h_ML, CS)
    assert n == 1
    for m, (t0, t1) in enumerate(zip(before, tr)):
        a, b = inventory(g, h, t0), inventory(g, h, t1)
        assert abs(a - b) <= 1e-12 * max(1.0, abs(a)), (m, a, b)      # every flux leaves one cell and enters its neighbour
    assert np.array_equal(interior(g, tr[-1]), interior(g, before[-1]))      # no differences, no fluxes: a constant keeps its bits
    assert not np.array_equal(interior(g, tr[0]), interior(g, before[0]))


def test_checker_no_flux_through_faces_with_an_empty_boundary_layer_or_land():
    g, h, tr, h_ML = case(ntr=1)
    CS = hc.HBDCS(g.H_subroundoff)
    hbl = h_ML.copy()
    hbl[5:9, 6:12] = 0.0      # no boundary layer in a block of columns
    orc.halo_update(g, hbl, _abi.POS_H)
    fl = []
    kx, ky, _, I, _ = hc.khdt_and_itts(g, 3600.0, 5.0e3)
    hc.hor_bnd_diffusion(g, h, I * kx, I * ky, [tr[0].copy()], hbl, CS, fluxes=fl)
    uF, vF = fl[0]
    assert np.abs(uF).max() > 0.0
    for j in range(g.jsc, g.jec + 1):
        for I_ in range(g.isc - 1, g.iec + 1):
            if hbl[j - 1, I_ - 1] == 0.0 or hbl[j - 1, I_] == 0.0 or g.mask2dCu[j - 1, I_] == 0.0:
                assert not uF[:, j - 1, I_].any(), (I_, j)
    for J in range(g.jsc - 1, g.jec + 1):
        for i in range(g.isc, g.iec + 1):
            if hbl[J - 1, i - 1] == 0.0 or hbl[J, i - 1] == 0.0 or g.mask2dCv[J, i - 1] == 0.0:
                assert not vF[:, J, i - 1].any(), (i, J)
    # every layer whose centre lies below the shallower boundary layer carries nothing
    for j in range(g.jsc, g.jec + 1):
        for I_ in range(g.isc - 1, g.iec + 1):
            hL, hR = h[:, j - 1, I_ - 1], h[:, j - 1, I_]
            cL, cR = np.cumsum(hL) - 0.5 * hL, np.cumsum(hR) - 0.5 * hR
            deep = np.maximum(cL, cR) > min(hbl[j - 1, I_ - 1], hbl[j - 1, I_]) * (1 + 1e-12)
            assert not uF[deep, j - 1, I_].any()


def test_checker_handles_vanished_columns_and_deep_boundary_layers():
    g, h, tr, h_ML = case(ntr=1, hml=(1.5, 2.0))      # every boundary layer deeper than its column
    h = h.copy()
    h[:, 7, 8:11] = 0.0      # vanished columns (wet, but of no thickness)
    orc.halo_update(g, h, _abi.POS_H)
    t = [tr[0].copy()]
    hc.tracer_hordiff_hbd(g, h, 3600.0, t, 5.0e3, h_ML, hc.HBDCS(g.H_subroundoff))
    assert np.isfinite(interior(g, t[0])).all()
    assert abs(inventory(g, h, t[0]) - inventory(g, h, tr[0])) <= 1e-12 * abs(inventory(g, h, tr[0]))
    assert not np.array_equal(interior(g, t[0]), interior(g, tr[0]))


# ---- the library beside the checker (GPU) ---------------------------------------------------------------------------------------------
OPTS = [("default", {}), ("no_limiter", dict(APPLY_LIMITER=False)), ("limiter_remap", dict(APPLY_LIMITER_REMAP=True)),
        ("linear", dict(HBD_LINEAR_TRANSITION=True)), ("cfl_itts", dict(KhTr=6.0e7, CHECK_DIFFUSIVE_CFL=True, reentrant=(True, True))),
        ("underflow", dict(conc_underflow=[0.0, 0.0, 0.5], ntr=3, reentrant=(False, False)))] + \
       [(f"{s}{'_extrap' if e else ''}", dict(HBD_REMAPPING_SCHEME=s, HBD_BOUNDARY_EXTRAP=e)) for s in hc.SCHEMES for e in (False, True)
        if (s, e) != ("PLM", False)] + \
       [("along_layer_nk2", dict(nk=2, thin=False)), ("neutral_interior", dict(neutral=True)), ("neutral_cfl", dict(neutral=True, KhTr=2.0e7, max_diff_CFL=2.5)),
        ("nk40", dict(nk=40, ni=12, nj=8, HBD_REMAPPING_SCHEME="PPM_H4")), ("nk75", dict(nk=75, ni=10, nj=6)),
        ("nk100", dict(nk=100, ni=10, nj=6, HBD_REMAPPING_SCHEME="PPM_IH4", HBD_BOUNDARY_EXTRAP=True))] + \
       [  # the shortest columns of the serial drivers: where build_reconstructions_1d takes a lower scheme, and loops of a single turn
        ("nk4_cw_extrap", dict(nk=4, ni=10, nj=6, HBD_REMAPPING_SCHEME="PPM_CW", HBD_BOUNDARY_EXTRAP=True)),      # kept; one interior al
        ("nk4_ih4", dict(nk=4, ni=10, nj=6, HBD_REMAPPING_SCHEME="PPM_IH4")),      # taken as PPM_H4: one interior edge, both ends on the same cells
        ("nk5_ih4_extrap", dict(nk=5, ni=10, nj=6, HBD_REMAPPING_SCHEME="PPM_IH4", HBD_BOUNDARY_EXTRAP=True)),      # the smallest implicit solve, 6 rows
        ("nk3_h4_extrap", dict(nk=3, ni=10, nj=6, HBD_REMAPPING_SCHEME="PPM_H4", HBD_BOUNDARY_EXTRAP=True))]      # taken as PLM, extrapolated as PLM
HBD_KEYS = ("HBD_LINEAR_TRANSITION", "APPLY_LIMITER", "APPLY_LIMITER_REMAP", "HBD_BOUNDARY_EXTRAP", "HBD_REMAPPING_SCHEME")


@functools.lru_cache(maxsize=None)
def expected(name):
    """the case of OPTS[name] and the checker's HBD followed by orc.tracer_hordiff"""
    kw = dict(dict(OPTS)[name])
    gk = {k: kw.pop(k) for k in ("reentrant", "ni", "nj", "nk", "thin", "ntr") if k in kw}
    g, h, tr, h_ML = case(**gk)
    hk = {k: kw.pop(k) for k in HBD_KEYS if k in kw}
    KhTr, cfl = kw.pop("KhTr", 5.0e3), kw.pop("CHECK_DIFFUSIVE_CFL", False)
    mdc, cu, neutral = kw.pop("max_diff_CFL", -1.0), kw.pop("conc_underflow", None), kw.pop("neutral", False)
    assert not kw
    ref = [t.copy() for t in tr]
    n = hc.tracer_hordiff_hbd(g, h, 3600.0, ref, KhTr, h_ML, hc.HBDCS(g.H_subroundoff, **hk), max_diff_CFL=mdc, check_diffusive_CFL=cfl,
                              conc_underflow=cu)
    nd = dict(eos=orc.eos("WRIGHT"), idx_T=0, idx_S=1, h_ML=h_ML) if neutral else None
    st = orc.tracer_hordiff(g, h, 3600.0, ref, KhTr, max_diff_CFL=mdc, check_diffusive_CFL=cfl, conc_underflow=cu, neutral=nd)
    params = dict(KHTR=KhTr, MAX_TR_DIFFUSION_CFL=mdc, CHECK_DIFFUSIVE_CFL=cfl, USE_HORIZONTAL_BOUNDARY_DIFFUSION=True, **hk)
    if neutral:
        params.update(USE_NEUTRAL_DIFFUSION=True, NDIFF_INTERIOR_ONLY=True)
    return g, h, tr, h_ML, ref, (st.num_itts, st.halo_updates + n, st.max_CFL), params, cu


def run_library(g, h, tr, h_ML, params, cu, space, neutral):
    import torch
    from mom6_amd.tracer_advect import DeviceGrid
    from mom6_amd.tracer_hor_diff import tracer_hor_diff_init, tracer_hordiff
    dg = DeviceGrid(g)
    put = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if space == "device" else (lambda a: np.ascontiguousarray(a).copy())
    dtr = [put(t) for t in tr]
    CS = tracer_hor_diff_init(**params)
    tv = dict(T=dtr[0], S=dtr[1], eqn_of_state=orc.eos("WRIGHT")) if neutral else None
    st = tracer_hordiff(put(h), 3600.0, None, None, dict(h_ML=put(h_ML)), dg, CS, dtr, tv=tv, conc_underflow=cu)
    dg.sync()
    out = [a.cpu().numpy() if space == "device" else a for a in dtr]
    dg.close()
    return st, out


@pytest.mark.gpu
@pytest.mark.parametrize("name", [o[0] for o in OPTS])
@pytest.mark.parametrize("space", ["device", "host"])
def test_tracer_hordiff_hbd_matches_checker_bitwise(name, space):
    g, h, tr, h_ML, ref, stats, params, cu = expected(name)
    st, out = run_library(g, h, tr, h_ML, params, cu, space, params.get("USE_NEUTRAL_DIFFUSION", False))
    assert (st.num_itts, st.halo_updates, st.max_CFL) == stats
    bad = [m for m, (a, b) in enumerate(zip(out, ref)) if not bits_equal(interior(g, a), interior(g, b))]
    assert not bad, (bad, [float(np.abs(interior(g, out[m]) - interior(g, ref[m])).max()) for m in bad])
    assert not np.array_equal(interior(g, ref[0]), interior(g, tr[0]))


@pytest.mark.gpu
def test_tracer_hordiff_hbd_negative_zero_tracer_matches_checker():
    """a tracer of -0.0 in its deepest layer (below every boundary layer: no face carries a flux there), through HBD and the along-layer
    branch: the checker's bits.  (The reference's update of every wet layer turns -0.0 into +0.0; so does every later branch, so at this
    interface the two cannot be told apart -- hbd_update_kernel visits every layer of every wet cell all the same.)"""
    g, h, tr, h_ML, ref, stats, params, cu = expected("default")
    t = tr[0].copy()
    t[-1] = -0.0
    want = [t.copy(), tr[1].copy()]
    n = hc.tracer_hordiff_hbd(g, h, 3600.0, want, 5.0e3, h_ML, hc.HBDCS(g.H_subroundoff))
    orc.tracer_hordiff(g, h, 3600.0, want, 5.0e3)
    st, out = run_library(g, h, [t, tr[1]], h_ML, params, cu, "device", False)
    assert n == 1 and bits_equal(interior(g, out[0]), interior(g, want[0])) and bits_equal(interior(g, out[1]), interior(g, want[1]))


@pytest.mark.gpu
def test_tracer_hordiff_hbd_refuses_what_it_does_not_provide():
    import torch
    from mom6_amd import _lib
    from mom6_amd._lib import Mom6HipError
    from mom6_amd.tracer_advect import DeviceGrid
    from mom6_amd.tracer_hor_diff import tracer_hor_diff_init, tracer_hordiff
    import ctypes as C
    L = _lib.lib()
    L.mom6hip_abi_sizeof_hor_bnd_diffusion_cs.restype = C.c_uint64
    assert L.mom6hip_abi_sizeof_hor_bnd_diffusion_cs() == C.sizeof(_abi.HorBndDiffusionCS)
    g, h, tr, h_ML = case(ntr=2)
    dg = DeviceGrid(g)
    dh = torch.from_numpy(h).cuda(); dtr = [torch.from_numpy(t).cuda() for t in tr]
    visc = dict(h_ML=torch.from_numpy(h_ML).cuda())
    for s in ("PQM_IH4IH3", "PLM_HYBGEN", "WENO_HYBGEN"):
        with pytest.raises(Mom6HipError, match=f"HBD_REMAPPING_SCHEME = {s}"):
            tracer_hor_diff_init(KHTR=50.0, USE_HORIZONTAL_BOUNDARY_DIFFUSION=True, HBD_REMAPPING_SCHEME=s)
    with pytest.raises(Mom6HipError, match="HBD_DEBUG"):
        tracer_hordiff(dh, 3600.0, None, None, visc, dg, tracer_hor_diff_init(KHTR=50.0, USE_HORIZONTAL_BOUNDARY_DIFFUSION=True, HBD_DEBUG=True), dtr)
    with pytest.raises(Mom6HipError, match="USE_HORIZONTAL_BOUNDARY_DIFFUSION and DIFFUSE_ML_TO_INTERIOR are mutually exclusive"):
        tracer_hor_diff_init(KHTR=50.0, USE_HORIZONTAL_BOUNDARY_DIFFUSION=True, DIFFUSE_ML_TO_INTERIOR=True)
    with pytest.raises(Mom6HipError, match="hor_bnd_diffusion requires that visc%h_ML is associated"):
        tracer_hordiff(dh, 3600.0, None, None, None, dg, tracer_hor_diff_init(KHTR=50.0, USE_HORIZONTAL_BOUNDARY_DIFFUSION=True), dtr)
    CS = tracer_hor_diff_init(KHTR=50.0, USE_HORIZONTAL_BOUNDARY_DIFFUSION=True)
    CS.hor_bnd_diffusion_CSp.remap_scheme = _abi.REMAP_SCHEMES["PQM_IH6IH5"]      # past the Python mirror: the library refuses it too
    with pytest.raises(Mom6HipError, match="HBD_REMAPPING_SCHEME"):
        tracer_hordiff(dh, 3600.0, None, None, visc, dg, CS, dtr)
    # the entry points without the HBD control structure still refuse the flag
    cs = _abi.TracerHorDiffCS(); cs.KhTr = 50.0; cs.initialized = 1; cs.unsupported[1] = 1
    ptrs = (C.c_void_p * 2)(*[t.data_ptr() for t in dtr])
    L.mom6hip_tracer_hordiff.argtypes = [C.c_void_p, C.POINTER(_abi.TracerHorDiffCS), C.c_void_p, C.c_double, C.POINTER(C.c_void_p), C.c_void_p,
                                         C.c_int32, C.c_int32, C.POINTER(_abi.HorDiffStats)]
    rc = L.mom6hip_tracer_hordiff(dg.handle, C.byref(cs), C.c_void_p(dh.data_ptr()), 3600.0, ptrs, None, 2, _abi.MEM_DEVICE, C.byref(_abi.HorDiffStats()))
    assert rc != 0 and b"USE_HORIZONTAL_BOUNDARY_DIFFUSION" in L.mom6hip_last_error()
    dg.close()


def _write_case(tmp, g, h, tr, h_ML, kw, dt=3600.0, scheme="PPM:H3", resident=False):
    """the input and parameter files of tracer_driver.F90 (advect_tracer with zero transports, then tracer_hordiff with HBD), and the
    expectation: orc.advect_tracer, the checker's HBD, orc.tracer_hordiff"""
    kw = dict(kw)
    hk = {k: kw.pop(k) for k in ("HBD_LINEAR_TRANSITION", "APPLY_LIMITER", "APPLY_LIMITER_REMAP", "HBD_BOUNDARY_EXTRAP", "HBD_REMAPPING_SCHEME")
          if k in kw}
    KhTr, cfl, neutral = kw.pop("KhTr", 5.0e3), kw.pop("CHECK_DIFFUSIVE_CFL", False), kw.pop("neutral", False)
    uhtr, vhtr = np.zeros(g.shape3(_abi.POS_U)), np.zeros(g.shape3(_abi.POS_V))
    ref = [t.copy() for t in tr]
    orc.advect_tracer(g, h, uhtr, vhtr, dt, 900.0, scheme, ref)
    for t in ref:
        orc.halo_update(g, t, _abi.POS_H)
    hc.tracer_hordiff_hbd(g, h, dt, ref, KhTr, h_ML, hc.HBDCS(g.H_subroundoff, **hk), check_diffusive_CFL=cfl)
    orc.tracer_hordiff(g, h, dt, ref, KhTr, check_diffusive_CFL=cfl,
                       neutral=dict(eos=orc.eos("WRIGHT"), idx_T=0, idx_S=1, ndiff_answer_date=20240401, H_to_RZ=1035.0, h_ML=h_ML) if neutral else None)
    zero_h, zero_u, zero_v = g.zeros2(_abi.POS_H), g.zeros2(_abi.POS_U), g.zeros2(_abi.POS_V)
    opt = [len(tr), 0, 0, 0, 1, 0, 0, 0]
    with open(tmp / "in.bin", "wb") as fh:
        np.array([g.ni, g.nj, g.nk, g.halo, int(g.reentrant_x), int(g.reentrant_y), g.first_direction, 0], dtype="<i4").tofile(fh)
        np.array([g.Angstrom_H, g.H_subroundoff, g.dZ_subroundoff, g.H_to_Z, g.Z_to_H, g.g_Earth, g.Rho0, 900.0], dtype="<f8").tofile(fh)
        np.array(opt, dtype="<i4").tofile(fh)
        for n in _abi.ALL_METRICS:
            np.ascontiguousarray(g.metrics[n], dtype="<f8").tofile(fh)
        np.array([dt, 1.0], dtype="<f8").tofile(fh)
        for a in [h, uhtr, vhtr] + tr + [zero_h, zero_u, zero_v, zero_u, zero_v, zero_h, zero_h, h_ML]:
            np.ascontiguousarray(a, dtype="<f8").tofile(fh)
    with open(tmp / "params.txt", "w") as fh:
        fh.write(f"TRACER_ADVECTION_SCHEME = {scheme}\nDT = 900.0\nKHTR = {KhTr!r}\nCHECK_DIFFUSIVE_CFL = {cfl}\nGPU_RESIDENT_DYNAMICS = {resident}\n")
        fh.write("USE_HORIZONTAL_BOUNDARY_DIFFUSION = True\n")
        for k, v in hk.items():
            fh.write(f"{k} = {v}\n")
        if neutral:
            fh.write("USE_NEUTRAL_DIFFUSION = True\nNDIFF_ANSWER_DATE = 20240401\nEQN_OF_STATE = WRIGHT\nNDIFF_INTERIOR_ONLY = True\n")
    return ref


@pytest.mark.gpu
def test_tracer_module_shim_hbd_matches_checker(tmp_path):
    """tracer_hor_diff_init / tracer_hordiff of the module shim (MOM_tracer_hor_diff_hip.F90) with USE_HORIZONTAL_BOUNDARY_DIFFUSION, called
    from Fortran with the reference's argument lists (visc%h_ML, an ePBL control structure in diabatic_CSp: tests/fortran/hbd_tracer_driver.F90),
    staged and resident"""
    from test_fortran_abi import FC, _build_shims
    if not os.path.exists(FC):
        pytest.skip("amdflang not present")
    exe = _build_shims(tmp_path, driver="hbd_tracer_driver")
    g, h, tr, h_ML = case()
    for name, kw in [("default", {}), ("PPM_CW_extrap", dict(HBD_REMAPPING_SCHEME="PPM_CW", HBD_BOUNDARY_EXTRAP=True, APPLY_LIMITER_REMAP=True)),
                     ("neutral_interior", dict(neutral=True))]:
        for resident in (False, True):
            ref = _write_case(tmp_path, g, h, tr, h_ML, kw, resident=resident)
            r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(tmp_path / "params.txt")], capture_output=True, text=True)
            assert r.returncode == 0 and "tracer_driver ok" in r.stdout, (name, resident, r.stderr[-600:])
            raw = np.fromfile(str(tmp_path / "out.bin"), dtype="<f8").reshape((len(tr),) + tr[0].shape)
            for m, w in enumerate(ref):
                assert bits_equal(interior(g, raw[m]), interior(g, w)), (name, resident, m)


def test_tracer_module_shim_hbd_needs_a_boundary_layer_scheme(tmp_path):
    """hor_bnd_diffusion_init is FATAL unless diabatic_CSp has KPP or ePBL (:122-124): the plain tracer_driver gives the shim none"""
    from test_fortran_abi import FC, _build_shims
    if not os.path.exists(FC):
        pytest.skip("amdflang not present")
    exe = _build_shims(tmp_path, driver="tracer_driver")
    g, h, tr, h_ML = case()
    _write_case(tmp_path, g, h, tr, h_ML, {})
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(tmp_path / "params.txt")], capture_output=True, text=True)
    assert r.returncode != 0 and "Horizontal boundary diffusion is true, but no valid boundary layer scheme was found" in r.stderr


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.gpu
@pytest.mark.parametrize("neutral", [False, True], ids=["along_layer", "neutral_interior"])
@pytest.mark.parametrize("layout", [(1, 2), (2, 1)])
def test_tracer_hordiff_hbd_layout_independence(tmp_path, layout, neutral):
    """two tiles (the halo-1 pass of hbl, the faces on the tiles' edges, the pass of the tracers before every call) == one, to the bit"""
    import torch.multiprocessing as mp
    from mp_workers_hbd import hbd_layout_worker
    mp.spawn(hbd_layout_worker, args=(2, _free_port(), layout, str(tmp_path), neutral), nprocs=2, join=True)
    glob = np.load(tmp_path / "global.npz")
    assert glob["it"][0] > 1
    for r in range(2):
        t = np.load(tmp_path / f"tile{r}.npz")
        i0, j0, ni, nj, its = t["ij"]
        assert its == glob["it"][0]
        for m in range(2):
            a = t[f"arr_{m}"]; b = glob[f"arr_{m}"][:, j0:j0 + nj, i0:i0 + ni]
            assert np.array_equal(a.view(np.uint64), np.ascontiguousarray(b).view(np.uint64)), (layout, r, m)
