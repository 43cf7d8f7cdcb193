"""NDIFF_CONTINUOUS = False through Fortran (tests/fortran/ebt_tracer_driver.F90, unchanged: its parameter file carries every switch):
- the reference's own MOM_tracer_hor_diff.F90, MOM_neutral_diffusion.F90 and src/ALE, compiled unmodified, beside the checker
  (tests/ndiff_disc_checker.py): bitwise, on a closed and on a re-entrant domain, over the option table (needs the reference and amdflang);
- a few small cases of that run, recorded in tests/golden/ndiff_discontinuous.json, hold the checker everywhere;
- the module shim (mom6_amd/fortran/MOM_tracer_hor_diff_hip.F90) with a parameter file that sets only NDIFF_CONTINUOUS = False, and one
  with PPM_H4 and method 2, beside the checker (GPU)."""
import json
import os

import numpy as np
import pytest

import ndiff_disc_checker as dc
from helpers import bits_equal, interior
from mom6_amd import _abi
from oracle import orc
from test_ndiff_discontinuous import stratified
from test_ndiff_taper_ebt_reference import build_ref_driver, hexes, run
from test_reference_kernels import FC, REF

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "ndiff_discontinuous.json")
has_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src")) or not os.path.exists(FC), reason="the reference or amdflang is not present")

# each scheme, each position method, each DELTA_RHO_FORM, NDIFF_REF_PRES > 0, NDIFF_INTERIOR_ONLY, HARD_FAIL_HEFF = False, the symmetric
# answer date, three iterations with RECALC_NEUTRAL_SURF, LINEAR and WRIGHT; every entry but soft_fail runs with HARD_FAIL_HEFF = True
CASES = {
    "defaults": dict(),
    "ppm_h4_m1_linear": dict(NDIFF_REMAPPING_SCHEME="PPM_H4", NEUTRAL_POS_METHOD=1, eos="LINEAR", noise=0.3),      # (test_ndiff_discontinuous.py says why)
    "ppm_ih4_m2_local": dict(NDIFF_REMAPPING_SCHEME="PPM_IH4", NEUTRAL_POS_METHOD=2, DELTA_RHO_FORM="local_pressure"),
    "plm_m3_full": dict(DELTA_RHO_FORM="full"),
    "ppm_h4_m2_refpres": dict(NDIFF_REMAPPING_SCHEME="PPM_H4", NEUTRAL_POS_METHOD=2, NDIFF_REF_PRES=2.0e7),
    "interior": dict(interior=True, NDIFF_REMAPPING_SCHEME="PPM_H4"),
    "soft_fail_20240401": dict(HARD_FAIL_HEFF=False, NDIFF_ANSWER_DATE=20240401, NDIFF_REMAPPING_SCHEME="PPM_IH4"),
    "recalc_3itts": dict(KhTr=1.0e9, max_diff_CFL=2.5, recalc=True, NDIFF_X_TOL=1.0e-12, NDIFF_MAX_ITER=4),
}
GOLDEN_CASES = ("defaults", "ppm_ih4_m2_local", "interior")
_DISC = ("NDIFF_REMAPPING_SCHEME", "NEUTRAL_POS_METHOD", "DELTA_RHO_FORM", "NDIFF_DRHO_TOL", "NDIFF_X_TOL", "NDIFF_MAX_ITER", "HARD_FAIL_HEFF", "NDIFF_REF_PRES")


def inputs(reentrant=(True, False), kw=None, **gk):
    g, h, tr = stratified(reentrant=reentrant, ntr=2, noise=(kw or {}).get("noise", 1.0), **gk)
    h_ML = np.ascontiguousarray(np.clip(0.6 * np.random.default_rng(9).random(g.shape2(_abi.POS_H)) - 0.1, 0.0, 1.2) * h.sum(0))
    return g, h, tr, h_ML


def expectation(g, h, tr, h_ML, kw, scheme="PPM:H3", stats=None):
    """orc.advect_tracer with zero transports, then the checker's tracer_hordiff -> (the tracers, the parameters, dt, visc%h_ML given)"""
    kw = dict(kw)
    kw.pop("noise", None)      # (the inputs were drawn with it)
    eos, interior_only, recalc = kw.pop("eos", "WRIGHT"), kw.pop("interior", False), kw.pop("recalc", False)
    KhTr, mdc, date, dt = kw.pop("KhTr", 800.0), kw.pop("max_diff_CFL", -1.0), kw.pop("NDIFF_ANSWER_DATE", 20240101), 3600.0
    disc = {k: kw.pop(k) for k in _DISC if k in kw}
    assert not kw
    ref = [t.copy() for t in tr]
    orc.advect_tracer(g, h, np.zeros(g.shape3(_abi.POS_U)), np.zeros(g.shape3(_abi.POS_V)), dt, 900.0, scheme, ref)
    for t in ref:
        orc.halo_update(g, t, _abi.POS_H)
    dc.tracer_hordiff_neutral(g, h, dt, ref, KhTr, orc.eos(eos), max_diff_CFL=mdc, h_ML=h_ML if interior_only else None, recalc_neutral_surf=recalc,
                              NDIFF_ANSWER_DATE=date, stats=stats, **disc)
    params = dict(TRACER_ADVECTION_SCHEME=scheme, DT=900.0, KHTR=KhTr, MAX_TR_DIFFUSION_CFL=mdc, USE_NEUTRAL_DIFFUSION=True, NDIFF_CONTINUOUS=False,
                  NDIFF_ANSWER_DATE=date, EQN_OF_STATE=eos, NDIFF_INTERIOR_ONLY=interior_only, RECALC_NEUTRAL_SURF=recalc, **disc)
    return ref, params, dt, interior_only


def write_case(tmp, g, h, tr, h_ML, kw, resident=False, only=None):
    """the input and parameter files of ebt_tracer_driver.F90 and the expectation; only: the parameter file holds just these keys beside
    what the driver itself needs"""
    ref, params, dt, give_hml = expectation(g, h, tr, h_ML, kw)
    zero_h, zero_u, zero_v = g.zeros2(_abi.POS_H), g.zeros2(_abi.POS_U), g.zeros2(_abi.POS_V)
    opt = [len(tr), 0, 0, 0, int(give_hml), 0, 0, 0]
    with open(tmp / "in.bin", "wb") as fh:
        np.array([g.ni, g.nj, g.nk, g.halo, int(g.reentrant_x), int(g.reentrant_y), g.first_direction, 0], dtype="<i4").tofile(fh)
        np.array([g.Angstrom_H, g.H_subroundoff, g.dZ_subroundoff, g.H_to_Z, g.Z_to_H, g.g_Earth, g.Rho0, 900.0], dtype="<f8").tofile(fh)
        np.array(opt, dtype="<i4").tofile(fh)
        for n in _abi.ALL_METRICS:
            np.ascontiguousarray(g.metrics[n], dtype="<f8").tofile(fh)
        np.array([dt, 1.0], dtype="<f8").tofile(fh)
        for a in [h, np.zeros(g.shape3(_abi.POS_U)), np.zeros(g.shape3(_abi.POS_V))] + tr + [zero_h, zero_u, zero_v, zero_u, zero_v, zero_h, zero_h] + \
                ([h_ML] if give_hml else []):
            np.ascontiguousarray(a, dtype="<f8").tofile(fh)
    with open(tmp / "params.txt", "w") as fh:
        fh.write(f"GPU_RESIDENT_DYNAMICS = {resident}\n")
        for k, v in params.items():
            if only is None or k in only:
                fh.write(f"{k} = {v if isinstance(v, (bool, str, int)) else repr(v)}\n")
    return ref


@pytest.fixture(scope="module")
def ref_exe(tmp_path_factory):
    return build_ref_driver(tmp_path_factory.mktemp("ref_tracer_ndd"))


@has_ref
@pytest.mark.parametrize("topo", [(False, False), (True, False)], ids=["closed", "reentrant_x"])
def test_reference_discontinuous_equals_the_checker(tmp_path, ref_exe, topo):
    bad = []
    for name, kw in CASES.items():
        g, h, tr, h_ML = inputs(reentrant=topo, kw=kw)
        ref = write_case(tmp_path, g, h, tr, h_ML, kw)
        raw, r = run(ref_exe, tmp_path, g, tr)
        assert raw is not None, (name, r.stdout[-300:], r.stderr[-1500:])      # (a FATAL of the reference, HARD_FAIL_HEFF among them, ends here)
        for m, w in enumerate(ref):
            if not bits_equal(interior(g, raw[m]), interior(g, w)):
                bad.append((name, m, int((interior(g, raw[m]) != interior(g, w)).sum()), float(np.abs(interior(g, raw[m]) - interior(g, w)).max())))
        assert not np.array_equal(interior(g, ref[0]), interior(g, tr[0]))
    assert not bad, bad


@pytest.mark.parametrize("name", list(CASES))
def test_reference_table_inputs_are_not_trivial(name):
    g, h, tr, h_ML = inputs(kw=CASES[name])
    shares = {}
    expectation(g, h, tr, h_ML, CASES[name], stats=shares)
    assert shares["heff_share"] >= 0.05 and shares["inside_share"] >= 0.05, shares
    if CASES[name].get("NEUTRAL_POS_METHOD", 3) != 1:
        assert shares["max_iter"] > 1, shares


@has_ref
def test_reference_stops_where_the_checker_finds_a_negative_sublayer(tmp_path, ref_exe):
    """method 1 on the full-noise input with HARD_FAIL_HEFF = True: the checker raises, and the reference itself stops with its FATAL
    (with HARD_FAIL_HEFF = False both run to the end and agree to the bit)"""
    kw = dict(CASES["ppm_h4_m1_linear"], noise=1.0)
    g, h, tr, h_ML = inputs(kw=kw)
    with pytest.raises(dc.NegativeThickness):
        expectation(g, h, tr, h_ML, kw)
    ref = write_case(tmp_path, g, h, tr, h_ML, dict(kw, HARD_FAIL_HEFF=False))
    raw, r = run(ref_exe, tmp_path, g, tr)
    assert raw is not None and all(bits_equal(interior(g, raw[m]), interior(g, w)) for m, w in enumerate(ref))
    text = open(tmp_path / "params.txt").read().replace("HARD_FAIL_HEFF = False", "HARD_FAIL_HEFF = True")
    open(tmp_path / "params.txt", "w").write(text)
    raw, r = run(ref_exe, tmp_path, g, tr)
    assert raw is None and r.returncode != 0 and "Negative thicknesses in neutral diffusion" in r.stderr + r.stdout, r.stderr[-500:]


def golden_inputs():
    return inputs(ni=12, nj=8, nk=5)


def record_golden(exe, tmp, path=GOLDEN):
    """the reference's answers of GOLDEN_CASES on the 12 x 8 x 5 grid, as hex floats (run by hand where the reference is present)"""
    g, h, tr, h_ML = golden_inputs()
    out = {"grid": [g.ni, g.nj, g.nk], "source": "the reference's MOM_tracer_hor_diff.F90 under tests/fortran/ebt_tracer_driver.F90", "cases": {}}
    for name in GOLDEN_CASES:
        write_case(tmp, g, h, tr, h_ML, CASES[name])
        raw, r = run(exe, tmp, g, tr)
        assert raw is not None, r.stderr[-1500:]
        out["cases"][name] = [hexes(g, raw[m]) for m in range(len(tr))]
    with open(path, "w") as fh:
        fh.write('{"grid": %s, "source": %s, "cases": {\n' % (json.dumps(out["grid"]), json.dumps(out["source"])))      # a tracer a line
        fh.write(",\n".join(' %s: [\n%s\n ]' % (json.dumps(n), ",\n".join("  " + json.dumps(t) for t in c)) for n, c in out["cases"].items()))
        fh.write("\n}}\n")


@has_ref
def test_reference_still_gives_the_recorded_golden(tmp_path, ref_exe):
    record_golden(ref_exe, tmp_path, tmp_path / "again.json")
    assert json.load(open(tmp_path / "again.json"))["cases"] == json.load(open(GOLDEN))["cases"]


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_checker_gives_the_reference_recorded_answers(name):
    gold = json.load(open(GOLDEN))
    g, h, tr, h_ML = golden_inputs()
    assert gold["grid"] == [g.ni, g.nj, g.nk]
    ref = expectation(g, h, tr, h_ML, CASES[name])[0]
    for m, w in enumerate(ref):
        assert hexes(g, w) == gold["cases"][name][m], (name, m)
    assert not np.array_equal(interior(g, ref[0]), interior(g, tr[0]))


# ---- the module shim ---------------------------------------------------------------------------------------------------------------
_DRIVER_KEYS = ("TRACER_ADVECTION_SCHEME", "DT", "KHTR", "USE_NEUTRAL_DIFFUSION", "EQN_OF_STATE", "NDIFF_CONTINUOUS")


@pytest.mark.gpu
@pytest.mark.parametrize("name,only", [("defaults", _DRIVER_KEYS), ("ppm_h4_m2", None)])
def test_tracer_module_shim_discontinuous_matches_checker(tmp_path, name, only):
    """tracer_hor_diff_init / tracer_hordiff of MOM_tracer_hor_diff_hip.F90 from Fortran: a parameter file that sets only
    NDIFF_CONTINUOUS = False (the defaults: PLM, method 3, mid_pressure), and one with PPM_H4 and method 2"""
    from test_fortran_abi import _build_shims
    if not os.path.exists(FC):
        pytest.skip("amdflang not present")
    exe = _build_shims(tmp_path, driver="ebt_tracer_driver")
    g, h, tr, h_ML = inputs()
    kw = CASES["defaults"] if name == "defaults" else dict(NDIFF_REMAPPING_SCHEME="PPM_H4", NEUTRAL_POS_METHOD=2)
    for resident in (False, True):
        ref = write_case(tmp_path, g, h, tr, h_ML, kw, resident=resident, only=only)
        raw, r = run(exe, tmp_path, g, tr)
        assert raw is not None, (name, resident, r.stderr[-600:])
        for m, w in enumerate(ref):
            assert bits_equal(interior(g, raw[m]), interior(g, w)), (name, resident, m)


@pytest.mark.gpu
def test_tracer_module_shim_discontinuous_refuses_by_name(tmp_path):
    from test_fortran_abi import _build_shims
    if not os.path.exists(FC):
        pytest.skip("amdflang not present")
    exe = _build_shims(tmp_path, driver="ebt_tracer_driver")
    g, h, tr, h_ML = inputs(ni=10, nj=6, nk=5)
    for extra, word in ((dict(NDIFF_REMAPPING_SCHEME="PQM_IH4IH3"), "NDIFF_REMAPPING_SCHEME"), (dict(NEUTRAL_POS_METHOD=4), "NEUTRAL_POS_METHOD"),
                        (dict(NDIFF_BOUNDARY_EXTRAP=True), "NDIFF_BOUNDARY_EXTRAP"), (dict(REMAPPING_ANSWER_DATE=20181231), "REMAPPING_ANSWER_DATE"),
                        (dict(NEUTRAL_POS_METHOD=0), "NEUTRAL_POS_METHOD"), (dict(NEUTRAL_POS_METHOD=2, DELTA_RHO_FORM="full"), "DELTA_RHO_FORM = full"),
                        (dict(NDIFF_INTERIOR_ONLY=True, NDIFF_TAPERING=True), "NDIFF_TAPERING"), (dict(KHTR_USE_EBT_STRUCT=True), "KHTR_USE_EBT_STRUCT")):
        write_case(tmp_path, g, h, tr, h_ML, dict())
        kept = [line for line in open(tmp_path / "params.txt") if line.split("=")[0].strip() not in extra]
        with open(tmp_path / "params.txt", "w") as fh:
            fh.writelines(kept + [f"{k} = {v}\n" for k, v in extra.items()])
        raw, r = run(exe, tmp_path, g, tr)
        assert raw is None and r.returncode != 0 and word in r.stderr, (extra, r.stderr[-400:])
