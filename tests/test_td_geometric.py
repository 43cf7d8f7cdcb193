"""thickness_diffuse with KHTH_USE_EBT_STRUCT / FULL_DEPTH_KHTH_MIN, MEKE_GEOMETRIC and MEKE_GM_SRC_ALT
(src/parameterizations/lateral/MOM_thickness_diffuse.F90:262-268, :306-324, :446-468, :1022-1061, :1633-1652): the plain restatement
tests/td_checker.py is tied to the oracle with the switches off, keeps the rotational symmetry the reference claims for its newer forms,
and the library equals it bit for bit on the GPU.  tests/test_td_geometric_reference.py holds the checker to the reference's own module."""
import numpy as np
import pytest

import td_checker as tc
import test_thickness_diffuse as tt
from helpers import bits_equal, interior
from mom6_amd import _abi
from oracle import orc

H, U, V = _abi.POS_H, _abi.POS_U, _abi.POS_V
DT = 3600.0
OUTPUTS = ("h", "uhtr", "vhtr", "uhGM", "vhGM", "GM_src", "MEKE_Kh")


@pytest.mark.parametrize("name", list(tt.VARIANTS))
def test_checker_equals_the_oracle_with_the_switches_off(name):
    """what ties the checker to what is already pinned: every variant of tests/test_thickness_diffuse.py, bit for bit"""
    g, d = tt.case()
    ref, (kw, args, eos) = tt.run_oracle(g, d, name)
    a = dict(args)
    if "MEKE_GM_src" in a:
        a["MEKE_GM_src"] = np.full(g.shape2(H), 7.0)
    out = tc.thickness_diffuse(g, d["h"], np.zeros_like(d["u"]), np.zeros_like(d["v"]), d["T"], d["S"], None if eos is None else orc.eos(eos), DT, **kw, **a)
    for n in ("h", "uhtr", "vhtr", "uhGM", "vhGM"):
        assert bits_equal(out[n], ref[n]), (name, n)
    assert (out["GM_src"] is None) == (ref["GM_src"] is None)
    if ref["GM_src"] is not None:
        assert bits_equal(out["GM_src"], ref["GM_src"]), name


# ---- rotational symmetry: the quarter turn of tests/rotation.py -----------------------------------------------------------------------
VEC = (("uhtr", "vhtr"), ("uhGM", "vhGM"), ("slope_x", "slope_y"), ("u", "v"))
FACE = (("L2u", "L2v"), ("SN_u", "SN_v"), ("Res_fn_u", "Res_fn_v"), ("Depth_fn_u", "Depth_fn_v"))


def _symmetric(name):
    """the checker on the quarter-turned grid against the turned result of the checker, on the compute domain: which outputs are the same bits"""
    from rotation import rotate_grid
    from test_rotation_tracers_params import turn
    g, d = tt.case(14, 10, 4, land_frac=0.15, reentrant_x=False, reentrant_y=False)
    f = tc.geom_fields(g)
    out = tc.run_table(g, d, name, fields=f)[0]
    gt = rotate_grid(g)
    dturned, fturned = turn(d, VEC, FACE), turn(f, VEC, FACE)
    outt = tc.run_table(gt, dturned, name, fields=fturned)[0]
    want = turn({n: out[n] for n in OUTPUTS if out[n] is not None}, VEC, FACE)
    # (the turned transports are minus the old ones: a face without transport holds -0.0 there, so the face outputs are compared by value)
    eq = lambda n: bits_equal if n in ("h", "GM_src", "MEKE_Kh") else np.array_equal
    return {n: bool(eq(n)(interior(gt, outt[n], tc_pos(gt, outt[n])), interior(gt, want[n], tc_pos(gt, want[n])))) for n in want}


def tc_pos(g, a):
    return next(p for p in (H, U, V) if tuple(a.shape[-2:]) == tuple(g.shape2(p)))


def test_the_forms_that_claim_rotational_symmetry_keep_it():
    """MEKE_GEOMETRIC with the 2019 parentheses (:459-465) and MEKE_GM_SRC_ANSWER_DATE >= 20240601 (:1634-1642) with the slope bug off (the bug
    limits one sign only, :2355-2359): a quarter turn of the inputs turns the outputs, to the bit"""
    for name in ("geometric", "src_alt_2024_no_slope_bug", "all_three"):
        same = _symmetric(name)
        assert all(same.values()), (name, same)


def test_the_older_source_date_does_not_keep_the_symmetry():
    """(u + u + v + v summed left to right, :1645-1649: after the turn the pairs are other pairs) -- so the test above can tell the two apart"""
    same = _symmetric("src_alt_no_slope_bug")
    assert not same.pop("GM_src") and all(same.values()), same


# ---- the Python mirror ---------------------------------------------------------------------------------------------------------------
NEW_PARAMS = dict(KHTH_USE_EBT_STRUCT=True, FULL_DEPTH_KHTH_MIN=True, MEKE_GEOMETRIC=True, MEKE_GEOMETRIC_ALPHA=0.07, MEKE_GEOMETRIC_EPSILON=3.0e-7,
                  MEKE_GEOMETRIC_ANSWER_DATE=20200101, MEKE_GM_SRC_ALT=True, MEKE_GM_SRC_ANSWER_DATE=20240601, MEKE_GM_SRC_ALT_SLOPE_BUG=False)
SWITCH_SLOTS = (4, 5, 7)      # MEKE_GEOMETRIC, GM_src_alt, khth_use_ebt_struct: slots of `unsupported` that have become switches


def test_init_carries_each_new_parameter_and_sets_no_refusal_slot():
    from mom6_amd.thickness_diffuse import thickness_diffuse_init
    refused = lambda st: [n for n in range(10) if n not in SWITCH_SLOTS and st.unsupported[n]]
    st = thickness_diffuse_init(None, THICKNESSDIFFUSE=True, KHTH=100.0).st      # the reference's defaults
    assert not any(st.unsupported) and st.full_depth_khth_min == 0
    assert (st.MEKE_GEOMETRIC_alpha, st.MEKE_GEOMETRIC_epsilon, st.MEKE_GEOM_answer_date) == (0.05, 1.0e-7, 99991231)
    assert (st.MEKE_src_answer_date, st.MEKE_src_slope_bug) == (20240101, 1)
    carried = dict(KHTH_USE_EBT_STRUCT=lambda s: s.unsupported[7] == 1, FULL_DEPTH_KHTH_MIN=lambda s: s.full_depth_khth_min == 1,
                   MEKE_GEOMETRIC=lambda s: s.unsupported[4] == 1, MEKE_GEOMETRIC_ALPHA=lambda s: s.MEKE_GEOMETRIC_alpha == 0.07,
                   MEKE_GEOMETRIC_EPSILON=lambda s: s.MEKE_GEOMETRIC_epsilon == 3.0e-7, MEKE_GEOMETRIC_ANSWER_DATE=lambda s: s.MEKE_GEOM_answer_date == 20200101,
                   MEKE_GM_SRC_ALT=lambda s: s.unsupported[5] == 1, MEKE_GM_SRC_ANSWER_DATE=lambda s: s.MEKE_src_answer_date == 20240601,
                   MEKE_GM_SRC_ALT_SLOPE_BUG=lambda s: s.MEKE_src_slope_bug == 0)
    for n, v in NEW_PARAMS.items():
        kw = {n: v}
        if n == "FULL_DEPTH_KHTH_MIN":      # read only with the EBT structure and KHTH_MIN > 0 (:2245)
            kw.update(KHTH_USE_EBT_STRUCT=True, KHTH_MIN=50.0)
        st = thickness_diffuse_init(None, THICKNESSDIFFUSE=True, KHTH=100.0, **kw).st
        assert carried[n](st), n
        assert refused(st) == [], n
    # ignored as the reference ignores it
    assert thickness_diffuse_init(None, KHTH=100.0, FULL_DEPTH_KHTH_MIN=True).st.full_depth_khth_min == 0
    assert thickness_diffuse_init(None, KHTH=100.0, FULL_DEPTH_KHTH_MIN=True, KHTH_USE_EBT_STRUCT=True).st.full_depth_khth_min == 0


# ---- GPU: the library against the checker ------------------------------------------------------------------------------------------------
SHAPES = [(12, 8, 2, 0.2, 0), (12, 8, 3, 0.2, 2), (70, 6, 5, 0.25, 0), (12, 8, 75, 0.2, 0)]      # (ni, nj, nk, land, nkml forced)
SENTINEL = -7.25e33
_REF = {}


def _reference(shape, name):
    """the checker's result for a shape and an entry of the table, computed once"""
    key = (shape, name)
    if key not in _REF:
        ni, nj, nk, land, nkml = shape
        g, d = tt.case(ni, nj, nk, land_frac=land, reentrant_x=True, reentrant_y=False)
        f = tc.geom_fields(g)
        _REF[key] = (g, d, f) + tc.run_table(g, d, name, fields=f, **(dict(nkml=nkml) if nkml else {}))
    return _REF[key]


def _library_call(dg, g, d, kw, args, eos, X):
    from mom6_amd.pressure_force import EOS_init
    from mom6_amd.thickness_diffuse import thickness_diffuse, thickness_diffuse_init
    pk = {tc.PARAMS[k]: v for k, v in kw.items() if k in tc.PARAMS}
    pk["KHTH_USE_EBT_STRUCT"] = "ebt_struct" in args
    CS = thickness_diffuse_init(dg, THICKNESSDIFFUSE=True, **pk)
    h, uhtr, vhtr = X(d["h"]), X(np.zeros_like(d["u"])), X(np.zeros_like(d["v"]))
    cdp = dict(uhGM=X(np.zeros_like(d["u"])), vhGM=X(np.zeros_like(d["v"])))
    meke = {}
    sj, si = g.csl(H)
    if "MEKE_Kh" in args:
        Kh0 = args["MEKE_Kh"].copy()
        if kw.get("MEKE_GEOMETRIC"):      # an output: what the call does not write must come back untouched
            Kh0[:] = SENTINEL; Kh0[sj, si] = args["MEKE_Kh"][sj, si]
        meke["Kh"] = X(Kh0)
    if "MEKE_MEKE" in args:
        meke["MEKE"] = X(args["MEKE_MEKE"])
    if "MEKE_GM_src" in args:
        src0 = np.full(g.shape2(H), SENTINEL); src0[sj, si] = 7.0
        meke["GM_src"] = X(src0)
    if "Rlay" in args:
        meke["Rlay"] = args["Rlay"]
    vm = {n: X(a) for n, a in args.items() if n in ("L2u", "L2v", "SN_u", "SN_v", "Res_fn_u", "Res_fn_v", "slope_x", "slope_y", "cg1", "Depth_fn_u",
                                                    "Depth_fn_v", "ebt_struct")}
    varmix = vm if kw.get("use_variable_mixing") else None
    tv = None if eos is None else (X(d["T"]), X(d["S"]), EOS_init(eos))
    thickness_diffuse(h, uhtr, vhtr, tv, DT, dg, meke, varmix, cdp, CS)
    dg.sync()
    return dict(h=h, uhtr=uhtr, vhtr=vhtr, uhGM=cdp["uhGM"], vhGM=cdp["vhGM"], GM_src=meke.get("GM_src"), MEKE_Kh=meke.get("Kh"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(tc.TABLE))
def test_gpu_equals_the_checker(name):
    """library == checker, bit for bit, on h, uhtr, vhtr, uhGM, vhGM, GM_src and MEKE%Kh, on device arrays and on staged host arrays: 12x8x2 (one
    interior interface), 12x8x3 with nkml = 2, 70x6x5 with land (a second, partly empty block of 64 lanes) and 12x8x75 (the production layer
    count).  The halos of GM_src and MEKE%Kh hold a sentinel before the call and after it."""
    import torch
    from mom6_amd.tracer_advect import DeviceGrid
    for shape in SHAPES:
        g, d, f, ref, kw, args, eos = _reference(shape, name)
        dg = DeviceGrid(g)
        for resident in (True, False):
            X = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if resident else (lambda a: np.ascontiguousarray(a).copy())
            N = (lambda a: a.cpu().numpy()) if resident else (lambda a: a)
            got = _library_call(dg, g, d, kw, args, eos, X)
            sj, si = g.csl(H)
            for n in OUTPUTS:
                if ref[n] is None:
                    continue
                a = N(got[n])
                if n in ("GM_src", "MEKE_Kh") and (n == "GM_src" or kw.get("MEKE_GEOMETRIC")):
                    halo = np.ones(a.shape, bool); halo[sj, si] = False
                    assert np.all(a[halo] == SENTINEL), (name, shape, resident, n, "halo written")
                    a, w = a[sj, si], ref[n][sj, si]
                else:
                    w = ref[n]
                assert bits_equal(a, w), (name, shape, resident, n, np.argwhere(a != w)[:3])
        dg.close()


@pytest.mark.gpu
def test_gpu_scratch_neighbours_are_untouched():
    """the planes the faces leave behind for MEKE_GM_SRC_ALT are scratch of the call; what lies beside the arrays of the call -- here the
    arrays themselves, allocated back to back with a sentinel layer on either side -- comes back untouched"""
    import torch
    from mom6_amd.pressure_force import EOS_init
    from mom6_amd.thickness_diffuse import thickness_diffuse, thickness_diffuse_init
    from mom6_amd.tracer_advect import DeviceGrid
    shape, name = SHAPES[2], "all_three"
    g, d, f, ref, kw, args, eos = _reference(shape, name)
    dg = DeviceGrid(g)

    def padded(a):
        big = torch.full((a.shape[0] + 2,) + a.shape[1:], SENTINEL, dtype=torch.float64, device="cuda")
        big[1:-1] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        return big
    bigs = {}

    def X(a):      # 3-D arrays get a sentinel layer on either side, 2-D arrays (GM_src, MEKE%Kh, MEKE%MEKE, SN_u ...) a sentinel row
        b = padded(a); bigs[len(bigs)] = b
        return b[1:-1]
    got = _library_call(dg, g, d, kw, args, eos, X)
    for b in bigs.values():
        assert bool((b[0] == SENTINEL).all()) and bool((b[-1] == SENTINEL).all())
    assert bits_equal(got["h"].cpu().numpy(), ref["h"])
    dg.close()


@pytest.mark.gpu
def test_gpu_still_refuses_by_name():
    import torch
    from mom6_amd._lib import Mom6HipError
    from mom6_amd.thickness_diffuse import thickness_diffuse, thickness_diffuse_init
    from mom6_amd.tracer_advect import DeviceGrid
    g, d = tt.case(12, 8, 3)
    dg = DeviceGrid(g)
    X = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def call(meke=None, varmix=None, **p):
        CS = thickness_diffuse_init(dg, THICKNESSDIFFUSE=True, KHTH=100.0, **p)
        thickness_diffuse(X(d["h"]), X(np.zeros_like(d["u"])), X(np.zeros_like(d["v"])), None, DT, dg, meke, varmix, None, CS)
    for p, word in ((dict(DETANGLE_INTERFACES=True), "DETANGLE_INTERFACES"), (dict(KH_ETA_CONST=1.0), "KH_ETA_CONST"), (dict(READ_KHTH=True), "READ_KHTH"),
                    (dict(USE_QG_LEITH_GM=True), "QG Leith"), (dict(USE_STANLEY_GM=True), "USE_STANLEY_GM"), (dict(USE_KH_IN_MEKE=True), "USE_KH_IN_MEKE"),
                    (dict(KHTH_MAX_CFL=0.0), "KHTH_MAX_CFL")):
        with pytest.raises(Mom6HipError, match=word):
            call(**p)
    with pytest.raises(Mom6HipError, match="USE_GME"):
        thickness_diffuse_init(dg, USE_GME=True)
    with pytest.raises(Mom6HipError, match="MEKE_GEOMETRIC_ANSWER_DATE"):
        thickness_diffuse_init(dg, MEKE_GEOMETRIC=True, MEKE_GEOMETRIC_ANSWER_DATE=20180101)
    f = tc.geom_fields(g)
    with pytest.raises(Mom6HipError, match="MEKE%MEKE"):
        call(meke=dict(Kh=X(f["MEKE_Kh"])), varmix=dict(SN_u=X(f["SN_u"]), SN_v=X(f["SN_v"])), MEKE_GEOMETRIC=True)
    with pytest.raises(Mom6HipError, match="SN_u"):
        call(meke=dict(Kh=X(f["MEKE_Kh"]), MEKE=X(f["MEKE_MEKE"])), MEKE_GEOMETRIC=True)
    with pytest.raises(Mom6HipError, match="ebt_struct"):
        call(varmix=dict(SN_u=X(f["SN_u"])), KHTH_USE_EBT_STRUCT=True)
    dg.close()
