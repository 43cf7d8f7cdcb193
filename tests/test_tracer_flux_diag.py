"""The tracer flux diagnostics on the GPU: ad_x, ad_y, ad2d_x, ad2d_y, advection_xy of advect_tracer (mom6hip_advect_tracer_diag) and df_x,
df_y, df2d_x, df2d_y of the along-layer tracer_hordiff (mom6hip_tracer_hordiff_diag) equal the numpy checker (tests/tracer_flux_checker.py)
bit for bit, over the WHOLE arrays (so what the library must not touch is compared too), on device arrays and on staged host arrays.

Shapes: ni = 20, 64, 70 (below, exactly and just above the 64-cell chunk of adv_x_kernel), nj = 5 (one adv_y segment) and 40 (four), nk = 3,
five tracers (a second group of the MAXG = 4 split).  Every array sits between two red zones that must come back untouched."""
import functools
import os

import numpy as np
import pytest

import tracer_flux_checker as fc
from helpers import bits_equal
from mom6_amd import _abi, synth
from mom6_amd._lib import Mom6HipError

pytestmark = pytest.mark.gpu
H, U, V = _abi.POS_H, _abi.POS_U, _abi.POS_V
DT, CS_DT, NTR, PAD, FILL, ZONE = 3600.0, 900.0, 5, 257, 7.0, -12345.0
POS = dict(ad_x=U, ad_y=V, ad2d_x=U, ad2d_y=V, advection_xy=H, df_x=U, df_y=V, df2d_x=U, df2d_y=V)
CU = [0.0, 0.0, 1.0e-3, 0.0, 0.0]
SHAPES = {"20x5": (20, 5, "PLM", True, True), "64x40": (64, 40, "PPM:H3", False, False), "70x12": (70, 12, "PPM", True, True),
          "30x40": (30, 40, "PPM", True, True)}


def shape_of(g, n):
    return g.shape2(POS[n]) if "2d" in n else g.shape3(POS[n])


@functools.lru_cache(maxsize=None)
def adv_case(key):
    """(grid, inputs, the checker's tracers and its five arrays for every tracer) -- formed once a shape and left unchanged"""
    ni, nj, scheme, x_first, rx = SHAPES[key]
    g = synth.make_grid(ni, nj, 3, seed=3, reentrant_x=rx)
    st = synth.make_advection_state(g, ntr=NTR, seed=4, hot_frac=0.05)
    A = dict(h_end=st["h_end"].numpy().copy(), uhtr=st["uhtr"].numpy().copy(), vhtr=st["vhtr"].numpy().copy(), tr=[t.numpy().copy() for t in st["tr"]])
    A["uhtr"][1, g.halo + 1:g.halo + 3, :] = 0.0; A["vhtr"][1, g.halo + 1:g.halo + 3, :] = 0.0      # rows with nothing to do from the start
    tr = [t.copy() for t in A["tr"]]
    diag = [{n: np.full(shape_of(g, n), FILL) for n in fc.ADV} for m in range(NTR)]
    a = fc.advect_tracer(g, A["h_end"], A["uhtr"], A["vhtr"], DT, CS_DT, scheme, tr, diag=diag, x_first=x_first, conc_underflow=CU)
    return g, A, tr, diag, a.log


def zoned(shape, device):
    """an array of FILL between two red zones -> (the whole buffer, the array: a contiguous view)"""
    n = int(np.prod(shape))
    if device:
        import torch
        buf = torch.full((n + 2 * PAD,), ZONE, dtype=torch.float64, device="cuda")
    else:
        buf = np.full(n + 2 * PAD, ZONE)
    a = buf[PAD:PAD + n].reshape(shape)
    a[...] = FILL
    return buf, a


def host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def zones_intact(buf):
    b = host(buf)
    return bool(np.all(b[:PAD] == ZONE) and np.all(b[-PAD:] == ZONE))


def wanted(which, names):
    """which -> {tracer: names}: 'all', 'first_and_last' (tracers 0 and 4: one of each group), or one array's name on every tracer"""
    if which == "all":
        return {m: names for m in range(NTR)}
    if which == "first_and_last":
        return {0: names, NTR - 1: names}
    return {m: (which,) for m in range(NTR)}


def run_advect(key, which, device):
    import torch
    from mom6_amd.tracer_advect import DeviceGrid, advect_tracer, tracer_advect_init
    g, A, tr_ref, diag_ref, _ = adv_case(key)
    _, _, scheme, x_first, _ = SHAPES[key]
    up = (lambda a: torch.from_numpy(a.copy()).cuda()) if device else (lambda a: a.copy())
    dg = DeviceGrid(g, device=0)
    try:
        tr = [up(t) for t in A["tr"]]
        bufs, diag = [], []
        for m in range(NTR):
            d = {}
            for n in wanted(which, fc.ADV).get(m, ()):
                b, a = zoned(shape_of(g, n), device); bufs.append(b); d[n] = a
            diag.append(d or None)
        advect_tracer(up(A["h_end"]), up(A["uhtr"]), up(A["vhtr"]), None, DT, dg, tracer_advect_init(CS_DT, scheme), tr, x_first_in=x_first,
                      conc_underflow=CU, diag=diag)
        dg.sync()
        plain = [up(t) for t in A["tr"]]
        advect_tracer(up(A["h_end"]), up(A["uhtr"]), up(A["vhtr"]), None, DT, dg, tracer_advect_init(CS_DT, scheme), plain, x_first_in=x_first,
                      conc_underflow=CU)
        dg.sync()
    finally:
        dg.close()
    bad = [("tracer", m) for m in range(NTR) if not bits_equal(host(tr[m]), tr_ref[m])]
    bad += [("tracer differs from the call without diagnostics", m) for m in range(NTR) if not bits_equal(host(tr[m]), host(plain[m]))]
    bad += [(n, m) for m in range(NTR) for n, a in (diag[m] or {}).items() if not bits_equal(host(a), diag_ref[m][n])]
    bad += [("red zone", q) for q, b in enumerate(bufs) if not zones_intact(b)]
    assert not bad, bad


@pytest.mark.parametrize("device", [True, False], ids=["device", "staged"])
@pytest.mark.parametrize("which", ["all", "first_and_last"])
@pytest.mark.parametrize("key", list(SHAPES))
def test_advect_tracer_diagnostics_equal_the_checker(key, which, device):
    run_advect(key, which, device)


@pytest.mark.parametrize("device", [True, False], ids=["device", "staged"])
@pytest.mark.parametrize("name", fc.ADV)
def test_each_advective_array_alone(name, device):
    run_advect("70x12", name, device)


@pytest.mark.parametrize("name", ["ad_y", "ad2d_y", "advection_xy"])
@pytest.mark.parametrize("key", ["30x40", "64x40"])
def test_each_meridional_array_alone_across_the_segments_of_adv_y(key, name):
    """nj = 40: four segments a block, so the face stores of a wave's first own row and the cells either side of a seam are compared"""
    run_advect(key, name, True)


def test_advection_inputs_reach_the_seams():
    """what the shapes above are for, from the checker's log: two iterations, rows idle from the start and rows that finish in the first"""
    for key in SHAPES:
        log = adv_case(key)[4]
        assert log["x_rows_skipped_at_start"] > 0 and log["y_rows_skipped_at_start"] > 0 and log["x_rows_done_after_first"] > 0, (key, log)
    assert adv_case("20x5")[4]["iterations"] >= 2 and adv_case("70x12")[4]["iterations"] >= 2


def test_general_advection_path_refuses_the_diagnostics_by_name(monkeypatch):
    from mom6_amd.tracer_advect import DeviceGrid, advect_tracer, tracer_advect_init
    g, A, _, _, _ = adv_case("20x5")
    monkeypatch.setenv("MOM6HIP_ADV_GENERIC", "1")
    dg = DeviceGrid(g, device=0)
    try:
        tr = [t.copy() for t in A["tr"]]
        diag = [dict(ad_x=np.zeros(g.shape3(U)))] + [None] * (NTR - 1)
        with pytest.raises(Mom6HipError, match="flux diagnostics.*general path"):
            advect_tracer(A["h_end"].copy(), A["uhtr"].copy(), A["vhtr"].copy(), None, DT, dg, tracer_advect_init(CS_DT, "PLM"), tr, diag=diag)
        advect_tracer(A["h_end"].copy(), A["uhtr"].copy(), A["vhtr"].copy(), None, DT, dg, tracer_advect_init(CS_DT, "PLM"), tr)      # without: as before
    finally:
        dg.close()


# ---- tracer_hordiff -------------------------------------------------------------------------------------------------------------------
HD_SHAPES = {"20x5": (20, 5, True), "70x12": (70, 12, False)}
HD_KW = dict(KhTr=5.0e4, max_diff_CFL=2.0)      # two iterations (:384)


@functools.lru_cache(maxsize=None)
def hd_case(key):
    from oracle import orc
    ni, nj, rx = HD_SHAPES[key]
    g = synth.make_grid(ni, nj, 3, seed=5, reentrant_x=rx)
    st = synth.make_advection_state(g, ntr=NTR, seed=6)
    h = st["h_end"].numpy().copy(); orc.halo_update(g, h, H)
    tr0 = [t.numpy().copy() for t in st["tr"]]
    tr = [t.copy() for t in tr0]
    diag = [{n: np.full(shape_of(g, n), FILL) for n in fc.DIFF} for m in range(NTR)]
    n_itt = fc.tracer_hordiff(g, h, DT, tr, diag=diag, conc_underflow=CU, **HD_KW)
    return g, h, tr0, tr, diag, n_itt


def run_hordiff(key, which, device):
    import torch
    from mom6_amd.tracer_advect import DeviceGrid
    from mom6_amd.tracer_hor_diff import tracer_hor_diff_init, tracer_hordiff
    g, h, tr0, tr_ref, diag_ref, n_itt = hd_case(key)
    up = (lambda a: torch.from_numpy(a.copy()).cuda()) if device else (lambda a: a.copy())
    dg = DeviceGrid(g, device=0)
    try:
        CS = tracer_hor_diff_init(KHTR=HD_KW["KhTr"], MAX_TR_DIFFUSION_CFL=HD_KW["max_diff_CFL"])
        tr = [up(t) for t in tr0]
        bufs, diag = [], []
        for m in range(NTR):
            d = {}
            for n in wanted(which, fc.DIFF).get(m, ()):
                b, a = zoned(shape_of(g, n), device); bufs.append(b); d[n] = a
            diag.append(d or None)
        st = tracer_hordiff(up(h), DT, None, None, None, dg, CS, tr, conc_underflow=CU, diag=diag)
        dg.sync()
        plain = [up(t) for t in tr0]
        tracer_hordiff(up(h), DT, None, None, None, dg, CS, plain, conc_underflow=CU)
        dg.sync()
    finally:
        dg.close()
    assert st.num_itts == n_itt == 2
    bad = [("tracer", m) for m in range(NTR) if not bits_equal(host(tr[m]), tr_ref[m])]
    bad += [("tracer differs from the call without diagnostics", m) for m in range(NTR) if not bits_equal(host(tr[m]), host(plain[m]))]
    bad += [(n, m) for m in range(NTR) for n, a in (diag[m] or {}).items() if not bits_equal(host(a), diag_ref[m][n])]
    bad += [("red zone", q) for q, b in enumerate(bufs) if not zones_intact(b)]
    assert not bad, bad


@pytest.mark.parametrize("device", [True, False], ids=["device", "staged"])
@pytest.mark.parametrize("which", ["all", "first_and_last"])
@pytest.mark.parametrize("key", list(HD_SHAPES))
def test_tracer_hordiff_diagnostics_equal_the_checker(key, which, device):
    run_hordiff(key, which, device)


@pytest.mark.parametrize("device", [True, False], ids=["device", "staged"])
@pytest.mark.parametrize("name", fc.DIFF)
def test_each_diffusive_array_alone(name, device):
    run_hordiff("70x12", name, device)


def _ts_case():
    """a state with tv%T, tv%S among the tracers, for the branches that need them"""
    from mom6_amd.pressure_force import EOS_init
    g, h, tr0, _, _, _ = hd_case("20x5")
    tr = [t.copy() for t in tr0]
    return g, h, tr, dict(T=tr[0], S=tr[1], eqn_of_state=EOS_init("WRIGHT"), P_Ref=2.0e7)


def test_neutral_diffusion_leaves_the_diffusive_arrays_zeroed():
    """USE_NEUTRAL_DIFFUSION: the along-layer loop does not run; the arrays are zero over the ranges of :389-406 and untouched elsewhere,
    and the tracers are those of the call without diagnostics"""
    from mom6_amd.tracer_advect import DeviceGrid
    from mom6_amd.tracer_hor_diff import tracer_hor_diff_init, tracer_hordiff
    g, h, tr, tv = _ts_case()
    dg = DeviceGrid(g, device=0)
    try:
        CS = tracer_hor_diff_init(KHTR=1000.0, USE_NEUTRAL_DIFFUSION=True)
        diag = [{n: np.full(shape_of(g, n), FILL) for n in fc.DIFF}] + [None] * (NTR - 1)
        tracer_hordiff(h.copy(), DT, None, None, None, dg, CS, tr, tv=tv, diag=diag)
        g2, h2, tr2, tv2 = _ts_case()
        tracer_hordiff(h2.copy(), DT, None, None, None, dg, tracer_hor_diff_init(KHTR=1000.0, USE_NEUTRAL_DIFFUSION=True), tr2, tv=tv2)
    finally:
        dg.close()
    assert all(bits_equal(a, b) for a, b in zip(tr, tr2))
    for n, a in diag[0].items():
        sj, si = g.csl(POS[n])
        want = np.full(shape_of(g, n), FILL); want[..., sj, si] = 0.0
        assert bits_equal(a, want), n


@pytest.mark.parametrize("device", [True, False], ids=["device", "staged"])
@pytest.mark.parametrize("ML_scale", [0.5, 0.0])
def test_diffuse_ml_interior_gives_df_x_and_df_y(ML_scale, device):
    """DIFFUSE_ML_TO_INTERIOR (nkml = 1, nk_rho_varies = 2): df_x and df_y equal the checker's, zero in the layers :544-550 leave out"""
    import torch
    from mom6_amd.tracer_advect import DeviceGrid
    from mom6_amd.tracer_hor_diff import tracer_hor_diff_init, tracer_hordiff
    g, h, tr, tv = _ts_case()
    want_tr = [t.copy() for t in tr]
    want = [{n: np.full(shape_of(g, n), FILL) for n in ("df_x", "df_y")} for m in range(NTR)]
    fc.tracer_hordiff(g, h, DT, want_tr, diag=want, Diffuse_ML_interior=(1, 2, ML_scale), **HD_KW)
    up = (lambda a: torch.from_numpy(a.copy()).cuda()) if device else (lambda a: a)
    tr = [up(t) for t in tr]; tv["T"], tv["S"] = tr[0], tr[1]
    bufs, diag = [], []
    for m in range(NTR):
        d = {}
        for n in ("df_x", "df_y"):
            b, a = zoned(shape_of(g, n), device); bufs.append(b); d[n] = a
        diag.append(d)
    dg = DeviceGrid(g, device=0)
    try:
        CS = tracer_hor_diff_init(KHTR=HD_KW["KhTr"], MAX_TR_DIFFUSION_CFL=HD_KW["max_diff_CFL"], DIFFUSE_ML_TO_INTERIOR=True, ML_KHTR_SCALE=ML_scale)
        tracer_hordiff(up(h), DT, None, None, None, dg, CS, tr, tv=tv, GV=dict(Rlay=1025.0 + 0.5 * np.arange(g.nk), nkml=1, nk_rho_varies=2), diag=diag)
        dg.sync()
    finally:
        dg.close()
    bad = [(n, m) for m in range(NTR) for n, a in diag[m].items() if not bits_equal(host(a), want[m][n])]
    bad += [("red zone", q) for q, b in enumerate(bufs) if not zones_intact(b)]
    assert not bad, bad
    sj, si = g.csl(U)
    assert np.all(host(diag[0]["df_x"])[1][sj, si] == 0.0) and np.any(host(diag[0]["df_x"])[2][sj, si] != 0.0)


def test_refusals_of_the_diffusive_diagnostics_that_remain_are_by_name():
    """df2d_x / df2d_y with DIFFUSE_ML_TO_INTERIOR (the epipycnal contribution), and the arrays with USE_HORIZONTAL_BOUNDARY_DIFFUSION and
    the along-layer loop"""
    from mom6_amd.tracer_advect import DeviceGrid
    from mom6_amd.tracer_hor_diff import tracer_hor_diff_init, tracer_hordiff
    g, h, tr, tv = _ts_case()
    dg = DeviceGrid(g, device=0)
    try:
        diag = [dict(df2d_x=np.zeros(g.shape2(U)))] + [None] * (NTR - 1)
        CS = tracer_hor_diff_init(KHTR=1000.0, DIFFUSE_ML_TO_INTERIOR=True)
        with pytest.raises(Mom6HipError, match="df2d_x / df2d_y together with DIFFUSE_ML_TO_INTERIOR"):
            tracer_hordiff(h.copy(), DT, None, None, None, dg, CS, tr, tv=tv, GV=dict(Rlay=1025.0 + 0.5 * np.arange(g.nk), nkml=1, nk_rho_varies=2), diag=diag)
        CS = tracer_hor_diff_init(KHTR=1000.0, USE_HORIZONTAL_BOUNDARY_DIFFUSION=True)
        with pytest.raises(Mom6HipError, match="diffusive flux diagnostics.*USE_HORIZONTAL_BOUNDARY_DIFFUSION"):
            tracer_hordiff(h.copy(), DT, None, None, None, dg, CS, tr, diag=diag)
    finally:
        dg.close()


# ---- the module shims, through tests/fortran/tracer_flux_driver.F90 -------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim_exe(tmp_path_factory):
    import os
    from test_fortran_abi import FC, _build_shims
    if not os.path.exists(FC):
        pytest.skip("amdflang not present")
    return _build_shims(tmp_path_factory.mktemp("tracer_flux_shim"), driver="tracer_flux_driver")


@pytest.mark.parametrize("resident", [False, True], ids=["staged", "resident"])
def test_module_shims_equal_the_checker(tmp_path, shim_exe, resident):
    """advect_tracer and tracer_hordiff of the module shims from Fortran with the arrays associated -- all nine on every tracer, and a subset
    on tracers 0 and 2 -- equal the checker bit for bit on the compute domain; DIFFUSE_ML_TO_INTERIOR gives df_x and df_y"""
    import test_tracer_flux_diag_reference as rf
    from helpers import interior
    g, A = rf.flux_case(True, 0)
    for names, tracers, scheme in ((rf.NINE, None, "PPM"), (("ad2d_x", "advection_xy", "df_y", "df2d_x"), (0, 2), "PLM")):
        rf.write_flux_case(tmp_path, g, A, scheme, names=names, tracers=tracers, resident=resident)
        rf.run_driver(shim_exe, tmp_path)
        tr, diag = rf.read_flux_out(tmp_path, g, names, tracers)
        want_tr, want, _ = rf.checker_run(g, A, scheme, names, tracers)
        assert all(bits_equal(interior(g, a, H), interior(g, b, H)) for a, b in zip(tr, want_tr)), (names, resident)
        assert not rf.differing(g, diag, want, names), (names, resident)
    ml = (1, 2, 0.5)
    rf.write_flux_case(tmp_path, g, A, "PLM", names=("df_x", "df_y"), ml=ml, resident=resident)
    rf.run_driver(shim_exe, tmp_path)
    _, diag = rf.read_flux_out(tmp_path, g, ("df_x", "df_y"))
    _, want, _ = rf.checker_run(g, A, "PLM", ("df_x", "df_y"), ml=ml)
    assert not rf.differing(g, diag, want, ("df_x", "df_y")), resident


@pytest.mark.parametrize("what, word", [("generic", "general path"), ("epi_df2d", "df2d_x / df2d_y together with DIFFUSE_ML_TO_INTERIOR"), ("hbd", "hbd_")])
def test_module_shims_refuse_what_remains_by_name(tmp_path, shim_exe, what, word):
    import os
    import subprocess
    import test_tracer_flux_diag_reference as rf
    g, A = rf.flux_case(False, 0)
    env = dict(os.environ)
    if what == "generic":
        env["MOM6HIP_ADV_GENERIC"] = "1"; rf.write_flux_case(tmp_path, g, A, "PLM", names=("ad_x",))
    elif what == "epi_df2d":
        rf.write_flux_case(tmp_path, g, A, "PLM", names=("df2d_x",), ml=(1, 2, 0.5))
    else:
        rf.write_flux_case(tmp_path, g, A, "PLM", names=(), extra="USE_HORIZONTAL_BOUNDARY_DIFFUSION = True\n")
        raw = bytearray(open(tmp_path / "in.bin", "rb").read()); raw[28:32] = (1 << 9).to_bytes(4, "little")      # hdr(8): an hbd_dfx id
        open(tmp_path / "in.bin", "wb").write(bytes(raw))
    r = subprocess.run([shim_exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(tmp_path / "params.txt")], capture_output=True, text=True, env=env)
    assert r.returncode != 0 and "FATAL" in r.stderr and word in r.stderr, (what, r.stderr[-600:])
