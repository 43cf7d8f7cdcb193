"""KHTH_USE_EBT_STRUCT, MEKE_GEOMETRIC and MEKE_GM_SRC_ALT through Fortran (tests/fortran/td_geom_driver.F90):
- the reference's own MOM_thickness_diffuse.F90, compiled unmodified with its MOM_isopycnal_slopes, MOM_interface_heights, density integrals
  and equation of state, beside the checker (tests/td_checker.py): bitwise, on a closed and a zonally re-entrant domain (needs the reference
  and amdflang);
- three small cases (12x8x5) of that run, recorded as hex floats in tests/golden/thickness_diffuse_geometric.json, hold the checker everywhere;
- the inputs of every table entry are shown not to be trivial, from the statistics the checker returns;
- the module shim (mom6_amd/fortran/MOM_thickness_diffuse_hip.F90), staged and resident, beside the checker (GPU)."""
import json
import os
import subprocess

import numpy as np
import pytest

import td_checker as tc
import test_thickness_diffuse as tt
from helpers import bits_equal, interior
from mom6_amd import _abi
from test_reference_kernels import FC, REF, ROOT, STUBS

H, U, V = _abi.POS_H, _abi.POS_U, _abi.POS_V
DT = 3600.0
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "thickness_diffuse_geometric.json")
GOLDEN_CASES = ("ebt_full_depth_min", "src_alt_fgnv", "all_three")
has_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src")) or not os.path.exists(FC), reason="the reference or amdflang is not present")
NAMES = ("h", "uhtr", "vhtr", "uhGM", "vhGM", "GM_src", "MEKE_Kh")
POS = dict(h=H, uhtr=U, vhtr=V, uhGM=U, vhGM=V, GM_src=H, MEKE_Kh=H)
FIELD_ORDER = ("MEKE_Kh", "L2u", "L2v", "SN_u", "SN_v", "Res_fn_u", "Res_fn_v", "slope_x", "slope_y")


def small_case(reentrant_x):
    return tt.case(12, 8, 5, land_frac=0.2, reentrant_x=reentrant_x, reentrant_y=False)


def write_case(tmp, g, d, name, resident=False, only=None):
    """the input and parameter files of td_geom_driver for an entry of the table -> (the checker's result, which outputs the file holds)"""
    f = tc.geom_fields(g)
    out, kw, args, eos = tc.run_table(g, d, name, fields=f)
    opt = [int(eos is not None), int("MEKE_Kh" in args), int("L2u" in args), int("Res_fn_u" in args), int("slope_x" in args), int("MEKE_GM_src" in args),
           int(kw.get("nkml", 0)), int(bool(kw.get("use_variable_mixing")))]
    bits = int("cg1" in args) + 2 * int("Depth_fn_u" in args) + 4 * int("MEKE_MEKE" in args) + 8 * int("ebt_struct" in args)
    with open(tmp / "in.bin", "wb") as fh:
        np.array([g.ni, g.nj, g.nk, g.halo, int(g.reentrant_x), int(g.reentrant_y), g.first_direction, bits], dtype="<i4").tofile(fh)
        np.array([g.Angstrom_H, g.H_subroundoff, g.dZ_subroundoff, g.H_to_Z, g.Z_to_H, g.g_Earth, g.Rho0, DT], dtype="<f8").tofile(fh)
        np.array(opt, dtype="<i4").tofile(fh)
        for n in _abi.ALL_METRICS:
            np.ascontiguousarray(g.metrics[n], dtype="<f8").tofile(fh)
        for a in (d["h"], d["T"], d["S"], args.get("Rlay", 1025.0 + 0.5 * np.arange(g.nk))):
            np.ascontiguousarray(a, dtype="<f8").tofile(fh)
        for n in FIELD_ORDER + tuple(m for m in ("cg1", "Depth_fn_u", "Depth_fn_v", "MEKE_MEKE", "ebt_struct") if m in args):
            np.ascontiguousarray(f[n], dtype="<f8").tofile(fh)
    with open(tmp / "params.txt", "w") as fh:
        fh.write(f"THICKNESSDIFFUSE = True\nGPU_RESIDENT_DYNAMICS = {resident}\n")
        if eos is not None:
            fh.write(f"EQN_OF_STATE = {eos}\n")
        if only is not None:
            fh.write(only)
        else:
            if "ebt_struct" in args:
                fh.write("KHTH_USE_EBT_STRUCT = True\n")
            for k, v in kw.items():
                if k in tc.PARAMS and k != "nkml":
                    fh.write(f"{tc.PARAMS[k]} = {v if isinstance(v, (bool, int)) else repr(float(v))}\n")
    have = [n for n in NAMES if out[n] is not None]
    return out, have


def read_out(tmp, g, out, have):
    raw = np.fromfile(str(tmp / "out.bin"), dtype="<f8")
    want = [out[n] for n in have]
    assert raw.size == sum(w.size for w in want)
    return {n: a.reshape(w.shape) for n, a, w in zip(have, np.split(raw, np.cumsum([w.size for w in want])[:-1]), want)}


def build_ref_td_geom_driver(tmp):
    """(as build_ref_td_driver of tests/test_reference_kernels.py, with the new driver)"""
    flags = ["-cpp", "-fdefault-real-8", "-O0", "-ffp-contract=off", "-DREFERENCE_KERNELS", "-DREF_EOS", "-DREF_INTERFACE_HEIGHTS",
             f"-I{REF}/config_src/memory/dynamic_symmetric", f"-I{REF}/src/framework", f"-I{REF}/src/equation_of_state", f"-I{REF}/src/ALE",
             f"-I{STUBS}", f"-I{tmp}", "-J", str(tmp)]
    objs = []
    for src in [os.path.join(STUBS, "mom6_stubs.F90"), os.path.join(REF, "src/core/MOM_density_integrals.F90"),
                os.path.join(REF, "src/core/MOM_interface_heights.F90"), os.path.join(REF, "src/core/MOM_isopycnal_slopes.F90"),
                os.path.join(REF, "src/parameterizations/lateral/MOM_thickness_diffuse.F90"), os.path.join(ROOT, "tests", "fortran", "td_geom_driver.F90")]:
        o = os.path.join(str(tmp), os.path.basename(src)[:-4] + ".o")
        r = subprocess.run([FC, *flags, "-c", src, "-o", o], capture_output=True, text=True)
        assert r.returncode == 0, f"{src}:\n" + r.stderr[-3000:]
        objs.append(o)
    exe = os.path.join(str(tmp), "td_geom_ref_driver")
    r = subprocess.run([FC, *objs, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def ref_exe(tmp_path_factory):
    return build_ref_td_geom_driver(tmp_path_factory.mktemp("td_geom_ref"))


def run_reference(exe, tmp, g, d, name):
    out, have = write_case(tmp, g, d, name)
    r = subprocess.run([exe, str(tmp / "in.bin"), str(tmp / "out.bin"), str(tmp / "params.txt")], capture_output=True, text=True)
    assert r.returncode == 0 and "td_geom_driver ok" in r.stdout, (name, r.stdout[-200:], r.stderr[-1500:])
    return out, read_out(tmp, g, out, have)


@has_ref
@pytest.mark.parametrize("reentrant_x", [False, True], ids=["closed", "reentrant_x"])
def test_reference_equals_the_checker(tmp_path, ref_exe, reentrant_x):
    """the reference's own module, every entry of the table: h, uhtr, vhtr, uhGM, vhGM, GM_src and MEKE%Kh equal the checker's bit for bit on
    the compute domain (src_alt_fgnv is where N2_floor is not zero: FGNV_STRAT_FLOOR = 0.02 puts it above part of the stratification)"""
    g, d = small_case(reentrant_x)
    bad = []
    for name in tc.TABLE:
        out, got = run_reference(ref_exe, tmp_path, g, d, name)
        for n, a in got.items():
            if not bits_equal(interior(g, a, POS[n]), interior(g, out[n], POS[n])):
                bad.append((name, n))
    assert not bad, bad


def _hex(a):
    return [float(x).hex() for x in np.ascontiguousarray(a).ravel()]


def test_golden_holds_the_checker():
    """runs everywhere: the recorded results of the reference's own module (closed 12x8x5) against the checker, compute domain, to the bit"""
    with open(GOLDEN) as fh:
        gold = json.load(fh)
    g, d = small_case(False)
    assert set(gold) == set(GOLDEN_CASES)
    for name in GOLDEN_CASES:
        out = tc.run_table(g, d, name)[0]
        for n, rec in gold[name].items():
            assert _hex(interior(g, out[n], POS[n])) == rec, (name, n)


@has_ref
def test_golden_is_what_the_reference_gives(tmp_path, ref_exe):
    """re-records the golden cases from the reference's own module and compares with the file (MOM6HIP_REGOLD=1 writes it)"""
    g, d = small_case(False)
    new = {}
    for name in GOLDEN_CASES:
        out, got = run_reference(ref_exe, tmp_path, g, d, name)
        new[name] = {n: _hex(interior(g, a, POS[n])) for n, a in got.items()}
    if os.environ.get("MOM6HIP_REGOLD") == "1":
        with open(GOLDEN, "w") as fh:
            json.dump(new, fh, indent=0, sort_keys=True)
    with open(GOLDEN) as fh:
        assert json.load(fh) == new


# ---- the inputs are not trivial ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reentrant_x", [False, True], ids=["closed", "reentrant_x"])
def test_the_inputs_are_not_trivial(reentrant_x):
    """from the statistics of the checker, per table entry.  Why each threshold is reachable: ebt_struct is uniform in (0.05, 1) at every level,
    so the mean of two is never exactly 1; with KHTH = 600 and KHTH_MIN = 200 the floor binds where that mean is below 1/3 (about one
    interface in five) and not elsewhere; KHTH_SLOPE_MAX = 2e-5 lies inside the spread of the slopes of the synthetic state, which has both
    signs; MEKE%MEKE in (0.02, 8) over SN in (0, 1e-6) puts alpha*MEKE/SN on either side of the CFL cap of about 3e5 m2 s-1."""
    g, d = small_case(reentrant_x)
    res = {name: tc.run_table(g, d, name) for name in tc.TABLE}
    wet_cells = interior(g, g.mask2dT, H) > 0
    mu, mv = interior(g, g.mask2dCu, U) > 0, interior(g, g.mask2dCv, V) > 0
    four_wet = wet_cells & mu[:, 1:] & mu[:, :-1] & mv[1:, :] & mv[:-1, :]
    assert four_wet.sum() >= 10
    for name, (out, kw, args, eos) in res.items():
        s = out["stats"]
        if "ebt_struct" in args:
            assert s["wet_ifaces"] > 0 and s["kh_differs"] >= 0.5 * s["wet_ifaces"], name
        if name == "ebt_full_depth_min":
            assert s["floor_binds"] >= 0.05 * s["wet_ifaces"] and s["floor_free"] >= 0.05 * s["wet_ifaces"], name
        if kw.get("GM_src_alt"):
            assert s["slope_above"] >= 0.02 * s["slope_ifaces"] > 0 and s["slope_below"] >= 0.02 * s["slope_ifaces"], name
            assert np.all(interior(g, out["GM_src"], H)[four_wet] != 0.0), name
        if kw.get("MEKE_GEOMETRIC"):
            assert np.all((interior(g, out["MEKE_Kh"], H) != interior(g, args["MEKE_Kh"], H))[wet_cells]), name
        if name == "geometric":
            assert 0 < s["cfl_binds"] < s["wet_faces"], name
    src = lambda n: interior(g, res[n][0]["GM_src"], H)
    assert not bits_equal(src("src_alt"), src("src_alt_no_slope_bug"))          # the two slope-bug settings
    assert not bits_equal(src("src_alt"), src("src_alt_2024"))                  # the two answer dates
    assert not bits_equal(src("src_alt_fgnv"), src("src_alt"))


# ---- the module shim ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_module_shim_equals_the_checker(tmp_path):
    """thickness_diffuse_init + thickness_diffuse of the module shim from Fortran, staged and with GPU_RESIDENT_DYNAMICS: all three switches,
    and a parameter file that sets only KHTH_USE_EBT_STRUCT = True"""
    from test_fortran_abi import _build_shims
    if not os.path.exists(FC):
        pytest.skip("amdflang not present")
    exe = _build_shims(tmp_path, driver="td_geom_driver")
    g, d = small_case(True)
    for name, only in (("all_three", None), ("ebt", "KHTH_USE_EBT_STRUCT = True\nKHTH = 600.0\n")):
        for resident in (False, True):
            out, have = write_case(tmp_path, g, d, name, resident, only)
            r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(tmp_path / "params.txt")], capture_output=True, text=True)
            assert r.returncode == 0 and "td_geom_driver ok" in r.stdout, (name, resident, r.stderr[-800:])
            got = read_out(tmp_path, g, out, have)
            for n, a in got.items():
                assert bits_equal(interior(g, a, POS[n]), interior(g, out[n], POS[n])), (name, resident, n)


def test_module_shim_and_driver_compile(tmp_path):
    """MOM_thickness_diffuse_hip.F90 with the new parameters and tests/fortran/td_geom_driver.F90 compile against the stand-ins"""
    from test_fortran_abi import _build_shims
    if not os.path.exists(FC):
        pytest.skip("amdflang not present")
    assert os.path.exists(_build_shims(tmp_path, driver="td_geom_driver"))


@pytest.fixture(scope="module")
def shim_exe(tmp_path_factory):
    from test_fortran_abi import _build_shims
    if not os.path.exists(FC):
        pytest.skip("amdflang not present")
    return _build_shims(tmp_path_factory.mktemp("td_geom_shim"), driver="td_geom_driver")


@pytest.mark.parametrize("line, word", [("DETANGLE_INTERFACES = True", "DETANGLE_INTERFACES"), ("USE_GME = True", "USE_GME"),
                                        ("USE_KH_IN_MEKE = True", "USE_KH_IN_MEKE"), ("READ_KHTH = True", "READ_KHTH"),
                                        ("USE_STANLEY_GM = True", "USE_STANLEY_GM"), ("KH_ETA_CONST = 10.0", "KH_ETA_CONST"),
                                        ("MEKE_GEOMETRIC = True\nMEKE_GEOMETRIC_ANSWER_DATE = 20180101", "MEKE_GEOMETRIC_ANSWER_DATE")])
def test_module_shim_still_refuses_by_name(tmp_path, shim_exe, line, word):
    """thickness_diffuse_init of the module shim stops with FATAL and the parameter's name, before anything touches a GPU"""
    g, d = small_case(False)
    write_case(tmp_path, g, d, "ebt", only="KHTH = 600.0\n" + line + "\n")
    r = subprocess.run([shim_exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(tmp_path / "params.txt")], capture_output=True, text=True)
    assert r.returncode != 0 and "FATAL" in r.stderr and word in r.stderr, (line, r.stderr[-500:])
