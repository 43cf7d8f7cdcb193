"""The numpy checker of the tracer flux diagnostics (tests/tracer_flux_checker.py) on the CPU:
- its tracers equal the oracle's advect_tracer / tracer_hordiff bit for bit, with the diagnostics absent and present;
- its nine arrays equal those of the reference's OWN MOM_tracer_advect.F90 / MOM_tracer_hor_diff.F90 (tests/fortran/tracer_flux_driver.F90 on
  the stand-ins, built as tests/test_reference_kernels.py builds tracer_driver; needs the reference and amdflang): closed and x-re-entrant
  domains, all three schemes, x-first and y-first, one and two diffusion iterations, DIFFUSE_ML_TO_INTERIOR (df_x, df_y);
- two small cases recorded as hex in tests/golden/tracer_flux_diagnostics.json hold both ways: checker against golden everywhere, reference
  against golden where it can be built;
- the inputs are not trivial, and more than half of the faces carry a non-zero diagnostic in the reference's own arrays."""
import numpy as np
import pytest

import tracer_flux_checker as fc
from helpers import bits_equal
from mom6_amd import _abi, synth
from oracle import orc

H, U, V = _abi.POS_H, _abi.POS_U, _abi.POS_V
POS = dict(ad_x=U, ad_y=V, ad2d_x=U, ad2d_y=V, advection_xy=H, df_x=U, df_y=V, df2d_x=U, df2d_y=V)
DT, CS_DT, NTR = 3600.0, 900.0, 3
CU = [0.0, 0.0, 1.0e-3]


def shape_of(g, n):
    return g.shape2(POS[n]) if "2d" in n else g.shape3(POS[n])


def adv_inputs(reentrant_x):
    g = synth.make_grid(24, 12, 3, seed=3, reentrant_x=reentrant_x)
    st = synth.make_advection_state(g, ntr=NTR, seed=4, hot_frac=0.05)
    A = dict(h_end=st["h_end"].numpy().copy(), uhtr=st["uhtr"].numpy().copy(), vhtr=st["vhtr"].numpy().copy(), tr=[t.numpy().copy() for t in st["tr"]])
    A["uhtr"][1, g.halo + 1:g.halo + 3, :] = 0.0; A["vhtr"][1, g.halo + 1:g.halo + 3, :] = 0.0
    return g, A


def run_checker(g, A, scheme, x_first, names):
    tr = [t.copy() for t in A["tr"]]
    diag = [{n: np.full(shape_of(g, n), 7.0) for n in names} for m in range(NTR)] if names else None
    a = fc.advect_tracer(g, A["h_end"], A["uhtr"], A["vhtr"], DT, CS_DT, scheme, tr, diag=diag, x_first=x_first, conc_underflow=CU)
    return tr, diag, a.log


@pytest.mark.parametrize("reentrant_x", [False, True], ids=["closed", "reentrant_x"])
@pytest.mark.parametrize("x_first", [True, False], ids=["x_first", "y_first"])
@pytest.mark.parametrize("scheme", ["PLM", "PPM:H3", "PPM"])
def test_checker_advection_equals_the_oracle(scheme, x_first, reentrant_x):
    g, A = adv_inputs(reentrant_x)
    ref = [t.copy() for t in A["tr"]]
    rs = orc.advect_tracer(g, A["h_end"], A["uhtr"], A["vhtr"], DT, CS_DT, scheme, ref, x_first=x_first, conc_underflow=CU)
    for names in ((), fc.ADV):
        tr, diag, log = run_checker(g, A, scheme, x_first, names)
        assert log["iterations"] == rs.iterations
        assert all(bits_equal(a, b) for a, b in zip(tr, ref)), (scheme, x_first, names)


@pytest.mark.parametrize("reentrant_x", [False, True], ids=["closed", "reentrant_x"])
def test_advective_arrays_hold_together(reentrant_x):
    g, A = adv_inputs(reentrant_x)
    _, diag, _ = run_checker(g, A, "PPM", True, fc.ADV)
    _, alone, _ = run_checker(g, A, "PPM", True, ("ad2d_y",))
    sj, si = g.csl(H)
    for m in range(NTR):
        d = diag[m]
        assert bits_equal(alone[m]["ad2d_y"], d["ad2d_y"])
        # the 2-D sums against the 3-D arrays: the same terms, but summed pass by pass, so equal to rounding only
        for a2, a3 in (("ad2d_x", "ad_x"), ("ad2d_y", "ad_y")):
            s = d[a3].sum(axis=0)
            assert np.allclose(d[a2], s, rtol=1e-12, atol=1e-12 * np.abs(d[a3]).max())
        # advection_xy = -div(ad) * IareaT wherever do_i held in every pass: to rounding on most cells, and never far off
        conv = -((d["ad_x"][:, sj, g.halo + 1:g.halo + g.ni + 1] - d["ad_x"][:, sj, g.halo:g.halo + g.ni])
                 + (d["ad_y"][:, g.halo + 1:g.halo + g.nj + 1, si] - d["ad_y"][:, g.halo:g.halo + g.nj, si])) * g.IareaT[sj, si]
        axy = d["advection_xy"][:, sj, si]
        close = np.isclose(axy, conv, rtol=1e-9, atol=1e-9 * np.abs(conv).max())
        assert close.mean() > 0.9, close.mean()


def test_the_advection_inputs_are_not_trivial():
    """two iterations; rows and layers idle from the start, others done after the first pass; land; and the share of faces of the compute
    domain that carry a non-zero diagnostic, stated and above one half"""
    for rx in (False, True):
        g, A = adv_inputs(rx)
        _, diag, log = run_checker(g, A, "PLM", True, fc.ADV)
        assert log["iterations"] >= 2, log
        assert log["x_rows_skipped_at_start"] > 0 and log["y_rows_skipped_at_start"] > 0, log
        assert log["x_rows_done_after_first"] > 0 and log["y_rows_done_after_first"] > 0, log
        assert (g.mask2dT[g.csl(H)] == 0).sum() > 0
        sju, siu = g.csl(U); sjv, siv = g.csl(V)
        share_x = float(np.mean(diag[0]["ad_x"][:, sju, siu] != 0.0)); share_y = float(np.mean(diag[0]["ad_y"][:, sjv, siv] != 0.0))
        print(f"reentrant_x={rx}: non-zero share of ad_x {share_x:.2f}, of ad_y {share_y:.2f}")
        assert share_x > 0.5 and share_y > 0.5, (share_x, share_y)


def hd_inputs(reentrant_x):
    g = synth.make_grid(24, 12, 4, seed=5, reentrant_x=reentrant_x)
    st = synth.make_advection_state(g, ntr=NTR, seed=6)
    h = st["h_end"].numpy().copy(); orc.halo_update(g, h, H)
    return g, h, [t.numpy().copy() for t in st["tr"]]


@pytest.mark.parametrize("reentrant_x", [False, True], ids=["closed", "reentrant_x"])
@pytest.mark.parametrize("kw, n_itt", [(dict(KhTr=1000.0), 1), (dict(KhTr=5.0e4, max_diff_CFL=2.0), 2), (dict(KhTr=5.0e4, max_diff_CFL=3.0, check_diffusive_CFL=True), None)])
def test_checker_diffusion_equals_the_oracle(kw, n_itt, reentrant_x):
    g, h, tr0 = hd_inputs(reentrant_x)
    ref = [t.copy() for t in tr0]
    rs = orc.tracer_hordiff(g, h, DT, ref, conc_underflow=CU, **kw)
    for names in ((), fc.DIFF):
        tr = [t.copy() for t in tr0]
        diag = [{n: np.full(shape_of(g, n), 7.0) for n in names} for m in range(NTR)] if names else None
        n = fc.tracer_hordiff(g, h, DT, tr, conc_underflow=CU, diag=diag, **kw)
        assert n == rs.num_itts and (n_itt is None or n == n_itt)
        assert all(bits_equal(a, b) for a, b in zip(tr, ref)), (kw, names)
        if names:
            sju, siu = g.csl(U)
            for m in range(NTR):
                d = diag[m]
                assert np.allclose(d["df2d_x"][sju, siu], d["df_x"][:, sju, siu].sum(axis=0), rtol=1e-12, atol=1e-12 * np.abs(d["df_x"]).max())
                assert np.all(d["df_x"][:, :g.halo, :] == 7.0)      # outside the ranges of :389-406 nothing is written
            share = float(np.mean(diag[0]["df_x"][:, sju, siu] != 0.0))
            print(f"non-zero share of df_x {share:.2f}")
            assert share > 0.5


def test_diffuse_ml_interior_leaves_its_layers_out():
    """DIFFUSE_ML_TO_INTERIOR (:544-550): with nkml = 1, nk_rho_varies = 2 layer 1 is scaled and layer 2 left out -- of the diagnostics too"""
    g, h, tr0 = hd_inputs(False)
    sju, siu = g.csl(U)
    out = {}
    for name, ml in (("plain", None), ("scaled", (1, 2, 0.5)), ("off", (1, 2, 0.0))):
        tr = [t.copy() for t in tr0]
        diag = [{n: np.full(shape_of(g, n), 7.0) for n in fc.DIFF} for m in range(NTR)]
        fc.tracer_hordiff(g, h, DT, tr, KhTr=5.0e4, max_diff_CFL=2.0, diag=diag, Diffuse_ML_interior=ml)
        out[name] = (tr, diag)
    for name in ("scaled", "off"):
        tr, diag = out[name]
        assert np.all(diag[0]["df_x"][1][sju, siu] == 0.0) and bits_equal(tr[0][1], tr0[0][1])
        assert bits_equal(diag[0]["df_x"][2:], out["plain"][1][0]["df_x"][2:])
    assert np.all(out["off"][1][0]["df_x"][0][sju, siu] == 0.0)
    assert np.any(out["scaled"][1][0]["df_x"][0][sju, siu] != 0.0) and not bits_equal(out["scaled"][1][0]["df_x"][0], out["plain"][1][0]["df_x"][0])


def test_abi_mirror_of_the_record():
    """mom6hip_tracer_flux_diag_t: nine pointers, advection first"""
    import ctypes as C
    assert C.sizeof(_abi.TracerFluxDiag) == 9 * C.sizeof(C.c_void_p)
    assert [n for n, _ in _abi.TracerFluxDiag._fields_] == list(_abi.ADV_DIAGS + _abi.DIFF_DIAGS)


# ---- the reference's own modules ------------------------------------------------------------------------------------------------------
import json
import os
import subprocess

from helpers import interior

NINE = fc.ADV + fc.DIFF
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "tracer_flux_diagnostics.json")
GOLDEN_CASES = {"closed_ppm_x_first": (False, "PPM", 0), "reentrant_plm_y_first": (True, "PLM", 1)}
HD = dict(KhTr=5.0e4, max_diff_CFL=2.0)


def flux_case(reentrant_x, first_direction, ni=24, nj=12):
    g = synth.make_grid(ni, nj, 3, seed=3, reentrant_x=reentrant_x)
    g.first_direction = first_direction; g._struct = None
    st = synth.make_advection_state(g, ntr=NTR, seed=4, hot_frac=0.05)
    A = dict(h_end=st["h_end"].numpy().copy(), uhtr=st["uhtr"].numpy().copy(), vhtr=st["vhtr"].numpy().copy(), tr=[t.numpy().copy() for t in st["tr"]])
    A["uhtr"][1, g.halo + 1:g.halo + 3, :] = 0.0; A["vhtr"][1, g.halo + 1:g.halo + 3, :] = 0.0
    return g, A


def checker_run(g, A, scheme, names=NINE, tracers=None, hd=HD, ml=None):
    """advect_tracer, then tracer_hordiff with the same thicknesses, as the driver runs them -> (tracers, the arrays by tracer, the log)"""
    tracers = range(NTR) if tracers is None else tracers
    tr = [t.copy() for t in A["tr"]]
    diag = [({n: np.full(shape_of(g, n), 7.0) for n in names} if m in tracers else None) for m in range(NTR)]
    adv = lambda d: None if d is None else {n: a for n, a in d.items() if n in fc.ADV}
    dif = lambda d: None if d is None else {n: a for n, a in d.items() if n in fc.DIFF}
    a = fc.advect_tracer(g, A["h_end"], A["uhtr"], A["vhtr"], DT, CS_DT, scheme, tr, diag=[adv(d) for d in diag])
    n_itt = fc.tracer_hordiff(g, A["h_end"], DT, tr, diag=[dif(d) for d in diag], Diffuse_ML_interior=ml, **hd)
    return tr, diag, dict(a.log, num_itts=n_itt)


def write_flux_case(tmp, g, A, scheme, names=NINE, tracers=None, hd=HD, resident=False, extra="", ml=None):
    """the input and parameter files of tests/fortran/tracer_flux_driver.F90 (the layout of tracer_driver's)"""
    import test_tracer_hor_diff as th
    tracers = range(NTR) if tracers is None else tracers
    f = th.varmix_fields(g)
    bits = sum(1 << NINE.index(n) for n in names)
    opt = [NTR, 0, 0, 0, 0, 0 if ml is None else ml[1], 0 if ml is None else ml[0], sum(1 << m for m in tracers)]
    with open(tmp / "in.bin", "wb") as fh:
        np.array([g.ni, g.nj, g.nk, g.halo, int(g.reentrant_x), int(g.reentrant_y), g.first_direction, bits], dtype="<i4").tofile(fh)
        np.array([g.Angstrom_H, g.H_subroundoff, g.dZ_subroundoff, g.H_to_Z, g.Z_to_H, g.g_Earth, g.Rho0, 900.0], dtype="<f8").tofile(fh)
        np.array(opt, dtype="<i4").tofile(fh)
        for n in _abi.ALL_METRICS:
            np.ascontiguousarray(g.metrics[n], dtype="<f8").tofile(fh)
        np.array([DT, 1.0], dtype="<f8").tofile(fh)
        for a in [A["h_end"], A["uhtr"], A["vhtr"]] + A["tr"] + [f[n] for n in ("Kh", "L2u", "L2v", "SN_u", "SN_v", "Res_fn_h", "Rd_dx_h")]:
            np.ascontiguousarray(a, dtype="<f8").tofile(fh)
        if ml is not None:
            np.array(list(1025.0 + 0.5 * np.arange(g.nk)) + [2.0e7], dtype="<f8").tofile(fh)
    with open(tmp / "params.txt", "w") as fh:
        fh.write(f"TRACER_ADVECTION_SCHEME = {scheme}\nDT = {CS_DT!r}\nKHTR = {hd['KhTr']!r}\nGPU_RESIDENT_DYNAMICS = {resident}\n")
        if "max_diff_CFL" in hd:
            fh.write(f"MAX_TR_DIFFUSION_CFL = {hd['max_diff_CFL']!r}\n")
        if ml is not None:
            fh.write(f"DIFFUSE_ML_TO_INTERIOR = True\nML_KHTR_SCALE = {ml[2]!r}\nEQN_OF_STATE = WRIGHT\n")
        fh.write(extra)


def read_flux_out(tmp, g, names=NINE, tracers=None):
    tracers = range(NTR) if tracers is None else tracers
    raw = np.fromfile(str(tmp / "out.bin"), dtype="<f8")
    n3 = int(np.prod(g.shape3(H)))
    tr = [raw[m * n3:(m + 1) * n3].reshape(g.shape3(H)) for m in range(NTR)]
    at, diag = NTR * n3, [None] * NTR
    for m in tracers:
        diag[m] = {}
        for n in NINE:
            if n in names:
                sz = int(np.prod(shape_of(g, n)))
                diag[m][n] = raw[at:at + sz].reshape(shape_of(g, n)); at += sz
    assert at == raw.size
    return tr, diag


def run_driver(exe, tmp, word="tracer_flux_driver ok"):
    r = subprocess.run([exe, str(tmp / "in.bin"), str(tmp / "out.bin"), str(tmp / "params.txt")], capture_output=True, text=True)
    assert r.returncode == 0 and word in r.stdout, (r.stdout[-200:], r.stderr[-1500:])


def differing(g, got, want, names):
    return [(m, n) for m in range(NTR) if want[m] for n in names if not bits_equal(interior(g, got[m][n], POS[n]), interior(g, want[m][n], POS[n]))]


@pytest.fixture(scope="module")
def ref_exe(tmp_path_factory):
    import test_reference_kernels as rk
    if not os.path.isdir(os.path.join(rk.REF, "src")) or not os.path.exists(rk.FC):
        pytest.skip("the reference or amdflang is not present")
    tmp = tmp_path_factory.mktemp("tracer_flux_ref")
    flags = ["-cpp", "-fdefault-real-8", "-O0", "-ffp-contract=off", "-DREFERENCE_KERNELS", "-DREF_EOS", "-DREF_INTERFACE_HEIGHTS", "-DREF_ALE",
             f"-I{rk.REF}/config_src/memory/dynamic_symmetric", f"-I{rk.REF}/src/framework", f"-I{rk.REF}/src/equation_of_state", f"-I{rk.REF}/src/ALE",
             f"-I{rk.STUBS}", f"-I{tmp}", "-J", str(tmp)]
    objs = []
    for src in [os.path.join(rk.STUBS, "mom6_stubs.F90")] + [os.path.join(rk.REF, r) for r in rk.TRACER_SOURCES] + \
               [os.path.join(rk.ROOT, "tests", "fortran", "tracer_flux_driver.F90")]:
        o = os.path.join(str(tmp), os.path.basename(src)[:-4] + ".o")
        r = subprocess.run([rk.FC, *flags, "-c", src, "-o", o], capture_output=True, text=True)
        assert r.returncode == 0, f"{src}:\n" + r.stderr[-3000:]
        objs.append(o)
    exe = os.path.join(str(tmp), "tracer_flux_ref_driver")
    r = subprocess.run([rk.FC, *objs, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("reentrant_x", [False, True], ids=["closed", "reentrant_x"])
@pytest.mark.parametrize("first_direction", [0, 1], ids=["x_first", "y_first"])
@pytest.mark.parametrize("scheme", ["PLM", "PPM:H3", "PPM"])
def test_reference_equals_the_checker(tmp_path, ref_exe, scheme, first_direction, reentrant_x):
    """the reference's own advect_tracer and tracer_hordiff with all nine arrays associated on every tracer: the tracers and the arrays equal
    the checker's bit for bit on the compute domain; the share of faces with a non-zero diagnostic, in the reference's arrays, is above 1/2"""
    g, A = flux_case(reentrant_x, first_direction)
    write_flux_case(tmp_path, g, A, scheme)
    run_driver(ref_exe, tmp_path)
    tr, diag = read_flux_out(tmp_path, g)
    want_tr, want, log = checker_run(g, A, scheme)
    assert log["iterations"] >= 2 or first_direction == 1 or not reentrant_x, log
    assert log["num_itts"] == 2
    assert all(bits_equal(interior(g, a, H), interior(g, b, H)) for a, b in zip(tr, want_tr))
    assert not differing(g, diag, want, NINE)
    for n in ("ad_x", "ad_y", "df_x", "df_y"):
        share = float(np.mean(interior(g, diag[0][n], POS[n]) != 0.0))
        print(f"{n}: non-zero on {share:.2f} of the faces (the reference's array)")
        assert share > 0.5, (n, share)


def test_reference_equals_the_checker_with_a_subset_and_one_iteration(tmp_path, ref_exe):
    """arrays on tracers 0 and 2 only, a subset of the nine, one diffusion iteration"""
    g, A = flux_case(True, 0)
    names = ("ad2d_x", "advection_xy", "df_y", "df2d_x")
    write_flux_case(tmp_path, g, A, "PPM", names=names, tracers=(0, 2), hd=dict(KhTr=1000.0))
    run_driver(ref_exe, tmp_path)
    tr, diag = read_flux_out(tmp_path, g, names, (0, 2))
    want_tr, want, log = checker_run(g, A, "PPM", names, (0, 2), hd=dict(KhTr=1000.0))
    assert log["num_itts"] == 1
    assert all(bits_equal(interior(g, a, H), interior(g, b, H)) for a, b in zip(tr, want_tr))
    assert not differing(g, diag, want, names)


@pytest.mark.parametrize("ML_scale", [0.5, 0.0])
def test_reference_diffuse_ml_interior_equals_the_checker(tmp_path, ref_exe, ML_scale):
    """DIFFUSE_ML_TO_INTERIOR with nkml = 1, nk_rho_varies = 2: df_x and df_y of the reference (the epipycnal diffusion that follows adds to
    the 2-D arrays and the tracers only, and is not restated by the checker) equal the checker's, the left-out layers included"""
    g, A = flux_case(False, 0)
    ml = (1, 2, ML_scale)
    write_flux_case(tmp_path, g, A, "PLM", names=("df_x", "df_y"), ml=ml)
    run_driver(ref_exe, tmp_path)
    _, diag = read_flux_out(tmp_path, g, ("df_x", "df_y"))
    _, want, _ = checker_run(g, A, "PLM", ("df_x", "df_y"), ml=ml)
    assert not differing(g, diag, want, ("df_x", "df_y"))
    sju, siu = g.csl(U)
    assert np.all(diag[0]["df_x"][1][sju, siu] == 0.0) and np.any(diag[0]["df_x"][2][sju, siu] != 0.0)
    assert np.any(diag[0]["df_x"][0][sju, siu] != 0.0) == (ML_scale > 0.0)


def _hex(a):
    return [float(x).hex() for x in np.ascontiguousarray(a).ravel()]


def golden_inputs(name):
    rx, scheme, fd = GOLDEN_CASES[name]
    g, A = flux_case(rx, fd, ni=10, nj=6)
    return g, A, scheme


def test_golden_holds_the_checker():
    """runs everywhere: the recorded arrays of the reference's own modules (tracer 0, compute domain) against the checker, to the bit"""
    with open(GOLDEN) as fh:
        gold = json.load(fh)
    assert set(gold) == set(GOLDEN_CASES)
    for name in GOLDEN_CASES:
        g, A, scheme = golden_inputs(name)
        _, want, _ = checker_run(g, A, scheme)
        for n in NINE:
            assert _hex(interior(g, want[0][n], POS[n])) == gold[name][n], (name, n)


def test_golden_is_what_the_reference_gives(tmp_path, ref_exe):
    """re-records the golden cases from the reference's own modules and compares with the file (MOM6HIP_REGOLD=1 writes it)"""
    new = {}
    for name in GOLDEN_CASES:
        g, A, scheme = golden_inputs(name)
        write_flux_case(tmp_path, g, A, scheme)
        run_driver(ref_exe, tmp_path)
        _, diag = read_flux_out(tmp_path, g)
        new[name] = {n: _hex(interior(g, diag[0][n], POS[n])) for n in NINE}
    if os.environ.get("MOM6HIP_REGOLD") == "1":
        with open(GOLDEN, "w") as fh:
            json.dump(new, fh, indent=0, sort_keys=True)
    with open(GOLDEN) as fh:
        assert json.load(fh) == new
