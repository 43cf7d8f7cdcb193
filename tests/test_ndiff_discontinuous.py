"""NDIFF_CONTINUOUS = False in tracer_hordiff (src/tracer/MOM_neutral_diffusion.F90:394-508, :1604-2255, :2442-2538).  The checker
(tests/ndiff_disc_checker.py) reproduces every known answer the reference holds for this branch (ndiff_unit_tests_discontinuous,
:2837-3086: its test_nsp cases and its five find_neutral_pos_linear answers, tests/golden/neutral_diffusion_discontinuous.json), as
test_nsp and test_rnp compare them; the library (mom6_amd/csrc/neutral_diffusion_disc.hip) is compared with the checker on the GPU,
bit for bit, and everything outside the scope is refused by name."""
import functools
import json
import os

import numpy as np
import pytest

import ndiff_disc_checker as dc
import test_neutral_diffusion as tnd
from helpers import bits_equal, interior
from mom6_amd import _abi
from oracle import orc

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "neutral_diffusion_discontinuous.json")))


# ---- the reference's known answers (no GPU) -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", GOLD["nsp"], ids=[f"{n}:{c['title']}" for n, c in enumerate(GOLD["nsp"])])
def test_find_neutral_surface_positions_discontinuous_known_answers(c):
    s = GOLD["setup"]
    nk = s["nk"]
    CS = dc.DiscCS(orc.eos(s["eos"]["form"], dRho_dT=s["eos"]["dRho_dT"], dRho_dS=s["eos"]["dRho_dS"]), NEUTRAL_POS_METHOD=s["neutral_pos_method"],
                   DELTA_RHO_FORM=s["delta_rho_form"], NDIFF_REF_PRES=s["ref_pres"])

    def pres(h):      # :2875-2881
        P = [[0., h[0]]]
        for k in range(1, nk):
            P.append([P[k - 1][1], P[k - 1][1] + h[k]])
        return P
    Pl, Pr = pres(s["hL"]), pres(s["hR"])
    Si = [[0., 0.] for _ in range(nk)]
    zero = [[0., 0.] for _ in range(nk)]
    stable_l = dc.mark_unstable_cells(CS, nk, c["TiL"], Si, Pl)
    stable_r = dc.mark_unstable_cells(CS, nk, c["TiR"], Si, Pr)
    PoL, PoR, KoL, KoR, hEff = dc.find_neutral_surface_positions_discontinuous(CS, nk, Pl, s["hL"], c["TiL"], Si, zero, zero, stable_l, Pr,
                                                                               s["hR"], c["TiR"], Si, zero, zero, stable_r)
    # test_nsp :3275: every entry differs from the answer by nothing
    assert KoL == c["KoL"] and KoR == c["KoR"]
    assert PoL == c["PoL"] and PoR == c["PoR"]
    assert hEff == c["hEff"]


@pytest.mark.parametrize("c", GOLD["rnp"], ids=[c["title"] for c in GOLD["rnp"]])
def test_find_neutral_pos_linear_known_answers(c):
    s = GOLD["rnp_setup"]
    CS = dc.DiscCS(orc.eos("LINEAR", dRho_dT=-1., dRho_dS=2.), NDIFF_MAX_ITER=s["max_iter"], NDIFF_DRHO_TOL=s["drho_tol"], NDIFF_X_TOL=s["x_tol"])
    pos = dc.find_neutral_pos_linear(CS, *c["args"], c["ppoly_T"], c["ppoly_S"])
    assert not abs(c["expected"] - pos) > 2 * np.finfo(np.float64).eps      # test_rnp :3336: within 2*EPSILON, as the reference compares


# ---- the 3-D branch ---------------------------------------------------------------------------------------------------------------------
def stratified(ni=26, nj=18, nk=6, seed=3, reentrant=(True, False), land_frac=0.2, ntr=3, noise=1.0):
    """test_neutral_diffusion.case without vanished layers, T and S made to decrease / increase with depth with noise small enough
    that most cells stay stable and large enough that a few do not (those are the marked-unstable cells of the walk)"""
    g, h, tr = tnd.case(ni=ni, nj=nj, nk=nk, seed=seed, reentrant=reentrant, land_frac=land_frac, ntr=3, thin=False)
    rng = np.random.default_rng(seed + 40)
    z = (np.arange(nk) / max(nk - 1, 1))[:, None, None]
    shape = h.shape
    T = np.ascontiguousarray(20.0 - 14.0 * z + 1.5 * np.sin(np.arange(shape[2]) / 3.0)[None, None, :] + 1.0 * np.cos(np.arange(shape[1]) / 2.0)[None, :, None]
                             + noise * (8.0 / nk) * rng.standard_normal(shape))
    S = np.ascontiguousarray(34.0 + 1.5 * z + noise * 0.1 * rng.standard_normal(shape))
    out = [T, S, tr[2]][:ntr]
    rng2 = np.random.default_rng(seed + 41)
    while len(out) < ntr:
        out.append(np.ascontiguousarray(rng2.random(shape) * g.mask2dT[None]))
    for t in out:
        orc.halo_update(g, t, _abi.POS_H)
    return g, h, out


# the option table: each scheme, each position method, each DELTA_RHO_FORM, NDIFF_REF_PRES > 0, NDIFF_INTERIOR_ONLY, HARD_FAIL_HEFF = False,
# the symmetric answer date, three iterations with RECALC_NEUTRAL_SURF, LINEAR and WRIGHT, and the shapes of the issue
DISC_CASES = {
    "defaults": dict(),
    # method 1 interpolates without the last position as a lower bound: with the full noise some sublayer goes negative and the reference
    # itself stops (test_ndiff_discontinuous_reference.py runs it); with less noise the entry runs to the end with HARD_FAIL_HEFF = True.
    # test_hard_fail_heff_returns_the_reference_message runs the full-noise input
    "ppm_h4_m1_linear": dict(NDIFF_REMAPPING_SCHEME="PPM_H4", NEUTRAL_POS_METHOD=1, eos="LINEAR", noise=0.3),
    "ppm_ih4_m2_local": dict(NDIFF_REMAPPING_SCHEME="PPM_IH4", NEUTRAL_POS_METHOD=2, DELTA_RHO_FORM="local_pressure"),
    "plm_m3_full": dict(DELTA_RHO_FORM="full"),
    "ppm_h4_m2_refpres": dict(NDIFF_REMAPPING_SCHEME="PPM_H4", NEUTRAL_POS_METHOD=2, NDIFF_REF_PRES=2.0e7),
    "interior": dict(interior=0.3, NDIFF_REMAPPING_SCHEME="PPM_H4"),
    "soft_fail_sym": dict(HARD_FAIL_HEFF=False, NDIFF_ANSWER_DATE=20240401, NDIFF_REMAPPING_SCHEME="PPM_IH4"),
    "recalc_3itts": dict(KhTr=1.0e9, max_diff_CFL=2.5, recalc_neutral_surf=True, reentrant=(True, True), NDIFF_X_TOL=1.0e-12, NDIFF_MAX_ITER=4),
    "nk2": dict(nk=2),
    "nk3": dict(nk=3, NDIFF_REMAPPING_SCHEME="PPM_IH4"),      # the fewest layers with a cell that is not a boundary cell (PPM falls back to PLM)
    "p_surf_70x9x3": dict(p_surf=True, reentrant=(False, False), ni=70, nj=9, nk=3, NDIFF_REMAPPING_SCHEME="PPM_H4"),
    "nk75": dict(ni=12, nj=8, nk=75, NDIFF_REMAPPING_SCHEME="PPM_IH4", NDIFF_ANSWER_DATE=20240401),
    "five_tracers": dict(ntr=5, conc_underflow=[0.0, 0.0, 0.5, 0.0, 0.0], NDIFF_ANSWER_DATE=20240401),
    # the order of 2024 and before with a partial second batch: the update from the fluxes [surface][face] (nd_update_kernel) with ns = 4 nk
    "five_tracers_2024": dict(ntr=5, conc_underflow=[0.0, 0.0, 0.5, 0.0, 0.0], NDIFF_ANSWER_DATE=20240330),
}
_DISC_KEYS = ("NDIFF_REMAPPING_SCHEME", "NEUTRAL_POS_METHOD", "DELTA_RHO_FORM", "NDIFF_DRHO_TOL", "NDIFF_X_TOL", "NDIFF_MAX_ITER", "HARD_FAIL_HEFF",
              "NDIFF_REF_PRES")


@functools.lru_cache(maxsize=None)
def expected(name):
    """the checker's answer for one entry of the table, computed once: (g, h, inputs, p_surf, h_ML, answer, statistics, shares)"""
    kw = dict(DISC_CASES[name])
    gk = {k: kw.pop(k) for k in ("reentrant", "ni", "nj", "nk", "ntr", "noise") if k in kw}
    g, h, tr = stratified(**gk)
    tr = tr + [np.full_like(tr[0], 3.5)]      # a constant tracer: it stays to the bit
    p_surf = np.ascontiguousarray(1.0e4 * np.random.default_rng(8).random(g.shape2(_abi.POS_H))) if kw.pop("p_surf", False) else None
    h_ML = None
    if "interior" in kw:
        frac = np.clip(kw.pop("interior") * 2.0 * np.random.default_rng(9).random(g.shape2(_abi.POS_H)) - 0.1, 0.0, 1.2)
        h_ML = np.ascontiguousarray(frac * h.sum(0))
    cu = kw.pop("conc_underflow", None)
    if cu is not None:
        cu = cu + [0.0]
    E = orc.eos(kw.pop("eos", "WRIGHT"))
    ref = [t.copy() for t in tr]
    shares = {}
    disc = {k: kw[k] for k in _DISC_KEYS if k in kw}
    st = dc.tracer_hordiff_neutral(g, h, 3600.0, ref, kw.get("KhTr", 800.0), E, max_diff_CFL=kw.get("max_diff_CFL", -1.0), conc_underflow=cu,
                                   p_surf=p_surf, h_ML=h_ML, recalc_neutral_surf=kw.get("recalc_neutral_surf", False),
                                   NDIFF_ANSWER_DATE=kw.get("NDIFF_ANSWER_DATE", 20240101), stats=shares, **disc)
    return g, h, tr, p_surf, h_ML, cu, E, ref, st, shares, kw, disc


@pytest.mark.parametrize("name", [n for n in DISC_CASES if n != "nk2"])
def test_checker_inputs_are_not_trivial(name):
    """every table entry runs to the end with HARD_FAIL_HEFF as it sets it (no negative sublayer), and the inputs exercise the walk: at
    least 5 % of the sublayers of the wet faces have hEff > 0, at least 5 % of the surfaces lie strictly inside a layer, and with
    method 2 or 3 some search iterates more than once.  The one reasoned exception is nk = 2:
    with nk = 2 build_reconstructions_1d makes both cells piecewise constant -- PLM's boundary cells -- so no cell is stable (delta_rho = 0
    is not > 0, :1855) and no sublayer has a thickness: the shares cannot be met there by any input; test_two_layers_diffuse_nothing)"""
    g, h, tr, p_surf, h_ML, cu, E, ref, st, shares, kw, disc = expected(name)
    assert shares["heff_share"] >= 0.05 and shares["inside_share"] >= 0.05, shares
    if disc.get("NEUTRAL_POS_METHOD", 3) != 1:
        assert shares["max_iter"] > 1, shares
    assert bits_equal(interior(g, ref[-1]), interior(g, tr[-1]))      # the constant tracer
    assert not np.array_equal(interior(g, ref[0]), interior(g, tr[0]))


def test_two_layers_diffuse_nothing():
    g, h, tr, p_surf, h_ML, cu, E, ref, st, shares, kw, disc = expected("nk2")
    assert shares["heff_share"] == 0.0 and all(bits_equal(interior(g, a), interior(g, b)) for a, b in zip(ref, tr))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DISC_CASES))
@pytest.mark.parametrize("space", ["device", "host"])
def test_tracer_hordiff_discontinuous_matches_checker_bitwise(name, space):
    import torch
    from mom6_amd.tracer_advect import DeviceGrid
    from mom6_amd.tracer_hor_diff import tracer_hor_diff_init, tracer_hordiff
    g, h, tr, p_surf, h_ML, cu, E, ref, rs, shares, kw, disc = expected(name)
    dg = DeviceGrid(g)
    put = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if space == "device" else (lambda a: np.ascontiguousarray(a).copy())
    dtr = [put(t) for t in tr]
    disc = dict(disc)
    disc.setdefault("NDIFF_REMAPPING_SCHEME", "PLM")
    CS = tracer_hor_diff_init(KHTR=kw.get("KhTr", 800.0), MAX_TR_DIFFUSION_CFL=kw.get("max_diff_CFL", -1.0), USE_NEUTRAL_DIFFUSION=True,
                              NDIFF_CONTINUOUS=False, NDIFF_ANSWER_DATE=kw.get("NDIFF_ANSWER_DATE", 20240101),
                              RECALC_NEUTRAL_SURF=kw.get("recalc_neutral_surf", False), NDIFF_INTERIOR_ONLY=h_ML is not None, **disc)
    tv = dict(T=dtr[0], S=dtr[1], eqn_of_state=E, p_surf=None if p_surf is None else put(p_surf))
    st = tracer_hordiff(put(h), 3600.0, None, None, None if h_ML is None else dict(h_ML=put(h_ML)), dg, CS, dtr, tv=tv, conc_underflow=cu)
    dg.sync()
    assert (st.num_itts, st.halo_updates) == rs[:2] and st.max_CFL == rs[2]
    for m, (a, b) in enumerate(zip(dtr, ref)):
        an = a.cpu().numpy() if space == "device" else a
        assert bits_equal(interior(g, an), interior(g, b)), m
    dg.close()


def test_checker_hard_fail_heff_on_the_method_1_input():
    kw = dict(DISC_CASES["ppm_h4_m1_linear"], HARD_FAIL_HEFF=True)
    kw.pop("noise")
    g, h, tr = stratified()
    with pytest.raises(dc.NegativeThickness, match="Negative thicknesses in neutral diffusion"):
        dc.tracer_hordiff_neutral(g, h, 3600.0, [t.copy() for t in tr], 800.0, orc.eos(kw.pop("eos")), **kw)


@pytest.mark.gpu
def test_hard_fail_heff_returns_the_reference_message():
    """an error code, not a fault: the kernel sets a bit of the `bad` word and carries on with the reset"""
    import torch
    from mom6_amd._lib import Mom6HipError
    from mom6_amd.tracer_advect import DeviceGrid
    from mom6_amd.tracer_hor_diff import tracer_hor_diff_init, tracer_hordiff
    g, h, tr = stratified()
    dg = DeviceGrid(g)
    dtr = [torch.from_numpy(t).cuda() for t in tr]
    CS = tracer_hor_diff_init(KHTR=800.0, USE_NEUTRAL_DIFFUSION=True, NDIFF_CONTINUOUS=False, NDIFF_REMAPPING_SCHEME="PPM_H4", NEUTRAL_POS_METHOD=1,
                              HARD_FAIL_HEFF=True)
    with pytest.raises(Mom6HipError, match="Negative thicknesses in neutral diffusion"):
        tracer_hordiff(torch.from_numpy(h).cuda(), 3600.0, None, None, None, dg, CS, dtr, tv=dict(T=dtr[0], S=dtr[1], eqn_of_state=orc.eos("LINEAR")))
    dg.close()


def _gpu_call(**params):
    import torch
    from mom6_amd.tracer_advect import DeviceGrid
    from mom6_amd.tracer_hor_diff import tracer_hor_diff_init, tracer_hordiff
    g, h, tr = stratified(ni=10, nj=6, nk=5, ntr=2, land_frac=0.0)
    dg = DeviceGrid(g)
    try:
        dtr = [torch.from_numpy(t).cuda() for t in tr]
        tv = dict(T=dtr[0], S=dtr[1], eqn_of_state=orc.eos("WRIGHT"))
        visc = dict(h_ML=torch.from_numpy(np.ascontiguousarray(0.2 * h.sum(0))).cuda())
        VarMix = dict(ebt_struct=torch.ones(g.shape3(_abi.POS_H), dtype=torch.float64, device="cuda")) if params.get("KHTR_USE_EBT_STRUCT") else None
        CS = tracer_hor_diff_init(KHTR=50.0, USE_NEUTRAL_DIFFUSION=True, NDIFF_CONTINUOUS=False, **params)
        tracer_hordiff(torch.from_numpy(h).cuda(), 3600.0, None, VarMix, visc, dg, CS, dtr, tv=tv)
    finally:
        dg.close()


REFUSALS = {
    "bare": (dict(), "NDIFF_CONTINUOUS"),
    "scheme": (dict(NDIFF_REMAPPING_SCHEME="PQM_IH4IH3"), "NDIFF_REMAPPING_SCHEME"),
    "scheme_ppm_cw": (dict(NDIFF_REMAPPING_SCHEME="PPM_CW"), "NDIFF_REMAPPING_SCHEME"),
    "boundary_extrap": (dict(NDIFF_REMAPPING_SCHEME="PLM", NDIFF_BOUNDARY_EXTRAP=True), "NDIFF_BOUNDARY_EXTRAP"),
    "remap_answer_date": (dict(NDIFF_REMAPPING_SCHEME="PLM", REMAPPING_ANSWER_DATE=20181231), "REMAPPING_ANSWER_DATE"),
    "pos_method_0": (dict(NDIFF_REMAPPING_SCHEME="PLM", NEUTRAL_POS_METHOD=0), "NEUTRAL_POS_METHOD"),
    "pos_method_4": (dict(NDIFF_REMAPPING_SCHEME="PLM", NEUTRAL_POS_METHOD=4), "NEUTRAL_POS_METHOD"),
    "method_2_full": (dict(NDIFF_REMAPPING_SCHEME="PLM", NEUTRAL_POS_METHOD=2, DELTA_RHO_FORM="full"), "NEUTRAL_POS_METHOD = 2 with DELTA_RHO_FORM = full"),
    "tapering": (dict(NDIFF_REMAPPING_SCHEME="PLM", NDIFF_INTERIOR_ONLY=True, NDIFF_TAPERING=True), "NDIFF_TAPERING"),
    "ebt_struct": (dict(NDIFF_REMAPPING_SCHEME="PLM", KHTR_USE_EBT_STRUCT=True), "KHTR_USE_EBT_STRUCT"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(REFUSALS))
def test_discontinuous_refuses_by_name(name):
    from mom6_amd._lib import Mom6HipError
    params, word = REFUSALS[name]
    with pytest.raises(Mom6HipError, match=word):
        _gpu_call(**params)


def test_abi_mirror_of_the_new_struct():
    import ctypes as C
    from mom6_amd import _lib
    L = _lib.lib()
    L.mom6hip_abi_sizeof_ndiff_discontinuous_cs.restype = C.c_uint64
    assert L.mom6hip_abi_sizeof_ndiff_discontinuous_cs() == C.sizeof(_abi.NdiffDiscontinuousCS)
    root = os.path.dirname(os.path.dirname(__file__))
    hdr = open(os.path.join(root, "include", "mom6hip.h")).read().split("typedef struct mom6hip_ndiff_discontinuous_cs")[1].split("}")[0]
    f90 = open(os.path.join(root, "mom6_amd", "fortran", "mom6hip_c_api.F90")).read().split(":: mom6hip_ndiff_discontinuous_cs_t")[1].split("end type")[0]
    import re
    names = [n for n, _ in _abi.NdiffDiscontinuousCS._fields_]
    # the three descriptions declare the same fields in the same order and with the same types (8-byte reals, then 4-byte integers)
    c_decl = re.findall(r"^\s*(double|int32_t)\s+(\w+)", hdr, re.M)
    assert [n for _, n in c_decl] == names
    assert [t for t, _ in c_decl] == ["double" if C.sizeof(t) % 8 == 0 and getattr(t, "_type_", t) in (C.c_double, "d") else "int32_t" for _, t in _abi.NdiffDiscontinuousCS._fields_]
    f_names = []
    for kind, rest in re.findall(r"^\s*(real\(c_double\)|integer\(c_int32_t\))\s*::\s*(.*)$", f90, re.M):
        f_names += [(kind.startswith("real"), m) for m in re.findall(r"(\w+)(?:\(\d+\))?\s*=", rest)]
    assert [n for _, n in f_names] == names
    assert [r for r, _ in f_names] == [t == "double" for t, _ in c_decl]
    assert [getattr(_abi.NdiffDiscontinuousCS, n).offset for n in names] == sorted(getattr(_abi.NdiffDiscontinuousCS, n).offset for n in names)


@pytest.mark.gpu
def test_library_refuses_in_its_own_words():
    """the C entry point itself, through ctypes: NDIFF_CONTINUOUS = False without the struct keeps the words it has always had; a scheme
    and a method outside the scope are refused by name by the library, not only by the mirror"""
    import ctypes as C
    import torch
    from mom6_amd import tracer_hor_diff as thd
    from mom6_amd._lib import Mom6HipError
    from mom6_amd.tracer_advect import DeviceGrid
    g, h, tr = stratified(ni=10, nj=6, nk=5, ntr=2, land_frac=0.0)
    dg = DeviceGrid(g)
    try:
        dtr = [torch.from_numpy(t).cuda() for t in tr]
        tv = dict(T=dtr[0], S=dtr[1], eqn_of_state=orc.eos("WRIGHT"))
        dh = torch.from_numpy(h).cuda()
        CS = thd.tracer_hor_diff_init(KHTR=50.0, USE_NEUTRAL_DIFFUSION=True, NDIFF_CONTINUOUS=False, NDIFF_REMAPPING_SCHEME="PLM")
        CS.discontinuous = False      # the struct stays behind: ndd = NULL
        with pytest.raises(Mom6HipError, match="NDIFF_CONTINUOUS = False is not provided by libmom6hip"):
            thd.tracer_hordiff(dh, 3600.0, None, None, None, dg, CS, dtr, tv=tv)
        for field, value, word in (("remap_scheme", _abi.REMAP_SCHEMES["PPM_CW"], "NDIFF_REMAPPING_SCHEME"), ("neutral_pos_method", 4, "NEUTRAL_POS_METHOD"),
                                   ("boundary_extrap", 1, "NDIFF_BOUNDARY_EXTRAP"), ("remap_answer_date", 20181231, "REMAPPING_ANSWER_DATE")):
            CS = thd.tracer_hor_diff_init(KHTR=50.0, USE_NEUTRAL_DIFFUSION=True, NDIFF_CONTINUOUS=False, NDIFF_REMAPPING_SCHEME="PLM")
            setattr(CS.ndiff_discontinuous, field, value)
            with pytest.raises(Mom6HipError, match=word):
                thd.tracer_hordiff(dh, 3600.0, None, None, None, dg, CS, dtr, tv=tv)
    finally:
        dg.close()
