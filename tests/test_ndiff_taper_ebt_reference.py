"""NDIFF_TAPERING, KHTR_USE_EBT_STRUCT and FULL_DEPTH_KHTR_MIN through Fortran (tests/fortran/ebt_tracer_driver.F90):
- the reference's own MOM_tracer_hor_diff.F90, MOM_neutral_diffusion.F90 and MOM_hor_bnd_diffusion.F90, compiled unmodified, beside the
  checker (tests/ndiff_checker.py, tests/hbd_ebt_checker.py): bitwise, on closed and re-entrant domains (needs the reference and amdflang);
- one small case of that run, recorded in tests/golden/ndiff_taper_ebt.json, holds the checker everywhere;
- the module shim (mom6_amd/fortran/MOM_tracer_hor_diff_hip.F90) with a parameter file that sets the switches, beside the checker (GPU)."""
import json
import os
import subprocess

import numpy as np
import pytest

import hbd_checker as hc
import hbd_ebt_checker as hec
import ndiff_checker as nc
import test_neutral_diffusion as tnd
from helpers import bits_equal, interior
from mom6_amd import _abi
from oracle import orc
from test_ndiff_taper_ebt import boundary_layer, ebt_structure
from test_reference_kernels import FC, REF, ROOT, STUBS, TRACER_SOURCES

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "ndiff_taper_ebt.json")
has_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src")) or not os.path.exists(FC), reason="the reference or amdflang is not present")

FLOOR = dict(KhTr=5.0e3, KhTr_min=2.0e3, dt=5.0)      # Coef(K) = 2.5e4 * ebt against KHTR_MIN = 2e3: floored where ebt < 0.08
CASES = {
    "taper": dict(neutral=True, taper=True), "ebt": dict(neutral=True, ebt=True, interior=False), "both": dict(neutral=True, taper=True, ebt=True),
    "both_20240401": dict(neutral=True, taper=True, ebt=True, date=20240401),
    "both_3itts": dict(neutral=True, taper=True, ebt=True, KhTr=1.0e9, max_diff_CFL=2.5),
    "hbd_ebt": dict(hbd=True, ebt=True), "hbd_ebt_khtr_min": dict(hbd=True, ebt=True, **FLOOR),
    "hbd_ebt_khtr_min_full_depth": dict(hbd=True, ebt=True, full=True, **FLOOR),
    "hbd_then_both": dict(hbd=True, neutral=True, taper=True, ebt=True, KhTr=5.0e3),
    "hbd_then_both_20240401_full_depth": dict(hbd=True, neutral=True, taper=True, ebt=True, full=True, date=20240401, **FLOOR),
}
GOLDEN_CASES = ("taper", "ebt", "both_20240401", "hbd_then_both_20240401_full_depth")


def inputs(reentrant=(True, False), **gk):
    g, h, tr = tnd.case(reentrant=reentrant, ntr=2, **gk)
    return g, h, tr, boundary_layer(g, h), ebt_structure(g, decay=4.0)


def expectation(g, h, tr, h_ML, ebt, kw, scheme="PPM:H3"):
    """orc.advect_tracer with zero transports, then the checker's tracer_hordiff -> (the tracers, the parameters, dt)"""
    kw = dict(kw)
    neutral, hbd, use_ebt, taper = kw.pop("neutral", False), kw.pop("hbd", False), kw.pop("ebt", False), kw.pop("taper", False)
    interior_only = kw.pop("interior", True) and neutral
    KhTr, KhTr_min, full, dt = kw.pop("KhTr", 800.0), kw.pop("KhTr_min", 0.0), kw.pop("full", False), kw.pop("dt", 3600.0)
    date, mdc = kw.pop("date", 20240101), kw.pop("max_diff_CFL", -1.0)
    assert not kw
    e = ebt if use_ebt else None
    ref = [t.copy() for t in tr]
    orc.advect_tracer(g, h, np.zeros(g.shape3(_abi.POS_U)), np.zeros(g.shape3(_abi.POS_V)), dt, 900.0, scheme, ref)
    for t in ref:
        orc.halo_update(g, t, _abi.POS_H)
    if hbd:
        hec.tracer_hordiff_hbd(g, h, dt, ref, KhTr, h_ML, hc.HBDCS(g.H_subroundoff), e, KhTr_min=KhTr_min, FULL_DEPTH_KHTR_MIN=full, max_diff_CFL=mdc)
    if neutral:
        nc.tracer_hordiff_neutral(g, h, dt, ref, KhTr, orc.eos("WRIGHT"), max_diff_CFL=mdc, h_ML=h_ML if interior_only else None, ebt_struct=e,
                                  KhTr_min=KhTr_min, NDIFF_TAPERING=taper, NDIFF_ANSWER_DATE=date, H_to_RZ=1035.0)
    else:      # the along-layer branch: level 1 of the coefficients, max(KHTR, KHTR_MIN) with VarMix%use_variable_mixing
        orc.tracer_hordiff(g, h, dt, ref, max(KhTr, KhTr_min), max_diff_CFL=mdc)
    params = dict(TRACER_ADVECTION_SCHEME=scheme, DT=900.0, KHTR=KhTr, KHTR_MIN=KhTr_min, MAX_TR_DIFFUSION_CFL=mdc, KHTR_USE_EBT_STRUCT=use_ebt,
                  FULL_DEPTH_KHTR_MIN=full, USE_HORIZONTAL_BOUNDARY_DIFFUSION=hbd, USE_NEUTRAL_DIFFUSION=neutral, NDIFF_ANSWER_DATE=date,
                  EQN_OF_STATE="WRIGHT", NDIFF_INTERIOR_ONLY=interior_only, NDIFF_TAPERING=taper)
    return ref, params, dt, (hbd or interior_only)


def write_case(tmp, g, h, tr, h_ML, ebt, kw, resident=False, give_ebt=True):
    """the input and parameter files of ebt_tracer_driver.F90 and the expectation"""
    ref, params, dt, give_hml = expectation(g, h, tr, h_ML, ebt, kw)
    use_ebt = bool(kw.get("ebt")) and give_ebt
    zero_h, zero_u, zero_v = g.zeros2(_abi.POS_H), g.zeros2(_abi.POS_U), g.zeros2(_abi.POS_V)
    opt = [len(tr), int(bool(kw.get("ebt"))), 0, 0, int(give_hml), 0, 0, int(use_ebt)]      # use_variable_mixing with the switch, as VarMix_init sets it
    with open(tmp / "in.bin", "wb") as fh:
        np.array([g.ni, g.nj, g.nk, g.halo, int(g.reentrant_x), int(g.reentrant_y), g.first_direction, 0], dtype="<i4").tofile(fh)
        np.array([g.Angstrom_H, g.H_subroundoff, g.dZ_subroundoff, g.H_to_Z, g.Z_to_H, g.g_Earth, g.Rho0, 900.0], dtype="<f8").tofile(fh)
        np.array(opt, dtype="<i4").tofile(fh)
        for n in _abi.ALL_METRICS:
            np.ascontiguousarray(g.metrics[n], dtype="<f8").tofile(fh)
        np.array([dt, 1.0], dtype="<f8").tofile(fh)
        for a in [h, np.zeros(g.shape3(_abi.POS_U)), np.zeros(g.shape3(_abi.POS_V))] + tr + [zero_h, zero_u, zero_v, zero_u, zero_v, zero_h, zero_h] + \
                ([h_ML] if give_hml else []) + ([ebt] if use_ebt else []):
            np.ascontiguousarray(a, dtype="<f8").tofile(fh)
    with open(tmp / "params.txt", "w") as fh:
        fh.write(f"GPU_RESIDENT_DYNAMICS = {resident}\n")
        for k, v in params.items():
            fh.write(f"{k} = {v if isinstance(v, (bool, str, int)) else repr(v)}\n")
    return ref


def run(exe, tmp, g, tr):
    r = subprocess.run([exe, str(tmp / "in.bin"), str(tmp / "out.bin"), str(tmp / "params.txt")], capture_output=True, text=True)
    if r.returncode != 0 or "tracer_driver ok" not in r.stdout:
        return None, r
    return np.fromfile(str(tmp / "out.bin"), dtype="<f8").reshape((len(tr),) + tr[0].shape), r


def build_ref_driver(tmp):
    """ebt_tracer_driver.F90 (-DREFERENCE_KERNELS) on the reference's own tracer modules, as test_reference_kernels.build_ref_tracer_driver"""
    flags = ["-cpp", "-fdefault-real-8", "-O0", "-ffp-contract=off", "-DREFERENCE_KERNELS", "-DREF_EOS", "-DREF_INTERFACE_HEIGHTS", "-DREF_ALE",
             f"-I{REF}/config_src/memory/dynamic_symmetric", f"-I{REF}/src/framework", f"-I{REF}/src/equation_of_state", f"-I{REF}/src/ALE",
             f"-I{STUBS}", f"-I{tmp}", "-J", str(tmp)]
    objs = []
    for src in [os.path.join(STUBS, "mom6_stubs.F90")] + [os.path.join(REF, r) for r in TRACER_SOURCES] + \
               [os.path.join(ROOT, "tests", "fortran", "ebt_tracer_driver.F90")]:
        o = os.path.join(str(tmp), os.path.basename(src)[:-4] + ".o")
        r = subprocess.run([FC, *flags, "-c", src, "-o", o], capture_output=True, text=True)
        assert r.returncode == 0, f"{src}:\n" + r.stderr[-3000:]
        objs.append(o)
    exe = os.path.join(str(tmp), "ebt_tracer_ref_driver")
    r = subprocess.run([FC, *objs, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def ref_exe(tmp_path_factory):
    return build_ref_driver(tmp_path_factory.mktemp("ref_tracer_ebt"))


def hexes(g, a):
    return [float(x).hex() for x in interior(g, a).ravel()]


@has_ref
@pytest.mark.parametrize("topo", [(False, False), (True, False)], ids=["closed", "reentrant_x"])
def test_reference_taper_and_ebt_equal_the_checker(tmp_path, ref_exe, topo):
    g, h, tr, h_ML, ebt = inputs(reentrant=topo)
    bad, outs = [], {}
    for name, kw in CASES.items():
        ref = write_case(tmp_path, g, h, tr, h_ML, ebt, kw)
        raw, r = run(ref_exe, tmp_path, g, tr)
        assert raw is not None, (name, r.stdout[-300:], r.stderr[-1500:])
        outs[name] = raw
        for m, w in enumerate(ref):
            if not bits_equal(interior(g, raw[m]), interior(g, w)):
                bad.append((name, m, int((interior(g, raw[m]) != interior(g, w)).sum()), float(np.abs(interior(g, raw[m]) - interior(g, w)).max())))
        assert not np.array_equal(interior(g, ref[0]), interior(g, tr[0]))
    assert not bad, bad
    # the switches and the floor are in play: each changes the reference's answer
    assert not np.array_equal(outs["taper"], outs["both"]) and not np.array_equal(outs["hbd_ebt_khtr_min"], outs["hbd_ebt_khtr_min_full_depth"])


def golden_inputs():
    return inputs(ni=12, nj=8, nk=4)


def record_golden(exe, tmp, path=GOLDEN):
    """the reference's answers of GOLDEN_CASES on the 12 x 8 x 4 grid, as hex floats (run by hand where the reference is present)"""
    g, h, tr, h_ML, ebt = golden_inputs()
    out = {"grid": [g.ni, g.nj, g.nk], "source": "the reference's MOM_tracer_hor_diff.F90 under tests/fortran/ebt_tracer_driver.F90", "cases": {}}
    for name in GOLDEN_CASES:
        write_case(tmp, g, h, tr, h_ML, ebt, CASES[name])
        raw, r = run(exe, tmp, g, tr)
        assert raw is not None, r.stderr[-1500:]
        out["cases"][name] = [hexes(g, raw[m]) for m in range(len(tr))]
    with open(path, "w") as fh:
        json.dump(out, fh, indent=0)


@has_ref
def test_reference_still_gives_the_recorded_golden(tmp_path, ref_exe):
    record_golden(ref_exe, tmp_path, tmp_path / "again.json")
    assert json.load(open(tmp_path / "again.json"))["cases"] == json.load(open(GOLDEN))["cases"]


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_checker_gives_the_reference_recorded_answers(name):
    gold = json.load(open(GOLDEN))
    g, h, tr, h_ML, ebt = golden_inputs()
    assert gold["grid"] == [g.ni, g.nj, g.nk]
    ref = expectation(g, h, tr, h_ML, ebt, CASES[name])[0]
    for m, w in enumerate(ref):
        assert hexes(g, w) == gold["cases"][name][m], (name, m)
    assert not np.array_equal(interior(g, ref[0]), interior(g, tr[0]))


# ---- the module shim ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_tracer_module_shim_taper_ebt_matches_checker(tmp_path):
    """tracer_hor_diff_init / tracer_hordiff of MOM_tracer_hor_diff_hip.F90 from Fortran with the reference's argument lists and a parameter
    file that sets KHTR_USE_EBT_STRUCT, FULL_DEPTH_KHTR_MIN and NDIFF_TAPERING; VarMix%ebt_struct staged and resident; FATAL without it"""
    from test_fortran_abi import _build_shims
    if not os.path.exists(FC):
        pytest.skip("amdflang not present")
    exe = _build_shims(tmp_path, driver="ebt_tracer_driver")
    g, h, tr, h_ML, ebt = inputs()
    for name in ("taper", "ebt", "both_20240401", "hbd_ebt_khtr_min", "hbd_ebt_khtr_min_full_depth", "hbd_then_both_20240401_full_depth"):
        for resident in (False, True):
            ref = write_case(tmp_path, g, h, tr, h_ML, ebt, CASES[name], resident=resident)
            raw, r = run(exe, tmp_path, g, tr)
            assert raw is not None, (name, resident, r.stderr[-600:])
            for m, w in enumerate(ref):
                assert bits_equal(interior(g, raw[m]), interior(g, w)), (name, resident, m)
    write_case(tmp_path, g, h, tr, h_ML, ebt, CASES["both"], give_ebt=False)
    raw, r = run(exe, tmp_path, g, tr)
    assert raw is None and r.returncode != 0 and "KHTR_USE_EBT_STRUCT needs VarMix%ebt_struct" in r.stderr
