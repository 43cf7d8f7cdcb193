"""tests/tracer_mix_checker.py, the numpy restatement of the twelve diagnostics neutral_diffusion and hor_bnd_diffusion post, held on the
CPU to what it is composed from and to what the arrays are: its tracers are the existing checkers' bit for bit in every case the GPU test
uses (tests/test_tracer_mix_diag.py), the 2-D arrays are the layer-ordered sums of the 3-D ones, the area-weighted content tendencies
vanish on closed and re-entrant domains (the fluxes only move tracer), and the inputs are such that every array has something in it."""
import numpy as np
import pytest

import hbd_checker as hc
import hbd_ebt_checker as hec
import ndiff_checker as nc
import ndiff_disc_checker as ndc
import tracer_mix_cases as tm
import tracer_mix_checker as mc
from helpers import bits_equal, interior
from mom6_amd import _abi
from oracle import orc

FILL, NTR, CU = tm.FILL, tm.NTR, tm.CU


def existing_checkers(name):
    """the tracers and statistics of the case from the checkers that were there before"""
    shape, kw = tm.CASES[name]
    g, I, _, _, _, _ = tm.expected(name)
    h, h_ML, ebt, dt = I["h"], I["h_ML"], I["ebt"], I["dt"]
    tr = [t.copy() for t in I["tr"]]
    KhTr = 5.0e3 if "hbd" in kw else 800.0
    KhTr_min, full, date = kw.get("KhTr_min", 0.0), kw.get("full", False), kw.get("date", 20240101)
    n = 0
    if "hbd" in kw:
        CS = hc.HBDCS(g.H_subroundoff, **kw["hbd"])
        if ebt is not None:
            n = hec.tracer_hordiff_hbd(g, h, dt, tr, KhTr, h_ML, CS, ebt, KhTr_min=KhTr_min, FULL_DEPTH_KHTR_MIN=full, conc_underflow=CU)
        else:
            n = hc.tracer_hordiff_hbd(g, h, dt, tr, KhTr, h_ML, CS, conc_underflow=CU)
    if not kw.get("neutral", True):
        st = orc.tracer_hordiff(g, h, dt, tr, max(KhTr, KhTr_min) if ebt is not None else KhTr, conc_underflow=CU)
        return tr, (st.num_itts, st.halo_updates + n, st.max_CFL)
    interior_only = bool(kw.get("interior", False) or kw.get("taper", False))
    if kw.get("disc"):
        st = ndc.tracer_hordiff_neutral(g, h, dt, tr, KhTr, orc.eos("WRIGHT"), conc_underflow=CU, p_surf=I["p_surf"],
                                        h_ML=h_ML if interior_only else None, NDIFF_ANSWER_DATE=date, **kw["disc"])
    else:
        st = nc.tracer_hordiff_neutral(g, h, dt, tr, KhTr, orc.eos("WRIGHT"), conc_underflow=CU, p_surf=I["p_surf"],
                                       h_ML=h_ML if interior_only else None, ebt_struct=ebt, KhTr_min=KhTr_min, NDIFF_ANSWER_DATE=date,
                                       NDIFF_TAPERING=kw.get("taper", False))
    return tr, (st[0], st[1] + n, st[2])


@pytest.mark.parametrize("name", list(tm.CASES))
def test_the_tracers_are_the_existing_checkers(name):
    g, I, tr, _, stats, _ = tm.expected(name)
    want, want_stats = existing_checkers(name)
    assert stats == want_stats
    bad = [m for m in range(NTR) if not bits_equal(interior(g, tr[m]), interior(g, want[m]))]
    assert not bad, bad
    assert not np.array_equal(interior(g, tr[0]), interior(g, I["tr"][0]))
    assert np.any((interior(g, tr[3]) == 0.0) & (interior(g, I["tr"][3]) != 0.0) & (interior(g, g.mask2dT)[None] > 0.))      # the underflow bites


@pytest.mark.parametrize("name", list(tm.CASES))
def test_what_the_arrays_are(name):
    g, I, _, mix, _, _ = tm.expected(name)
    h, Hs = I["h"], g.H_subroundoff
    area = interior(g, g.areaT)
    for m in range(NTR):
        D = mix[m]
        for n, a in D.items():      # nothing outside the compute range
            sj, si = g.csl(mc.POS[n])
            rest = a.copy(); rest[..., sj, si] = FILL
            assert np.all(rest == FILL), (n, m)
        for cont, c2d, conc, fx, fy in (("dfxy_cont", "dfxy_cont_2d", "dfxy_conc", None, None),
                                        ("hbdxy_cont", "hbdxy_cont_2d", "hbdxy_conc", "hbd_dfx", "hbd_dfy")):
            if cont not in D:
                continue
            t3 = interior(g, D[cont])
            s = np.zeros_like(t3[0])
            for k in range(g.nk):
                s = s + t3[k]
            assert bits_equal(interior(g, D[c2d]), s), (c2d, m)
            assert bits_equal(interior(g, D[conc]), t3 / (interior(g, h) + Hs)), (conc, m)
            assert np.all(t3[:, interior(g, g.mask2dT) == 0.] == 0.0)
            # the fluxes only move tracer: on a closed or re-entrant domain the area-weighted sum vanishes to roundoff
            total, scale = float((t3 * area[None]).sum()), float(np.abs(t3 * area[None]).sum())
            assert scale > 0.0 and abs(total) <= 1.0e-12 * scale, (cont, m, total, scale)
            if fx:
                for f3, f2 in ((fx, "hbd_dfx_2d"), (fy, "hbd_dfy_2d")):
                    pos = mc.POS[f3]
                    x3 = interior(g, D[f3], pos)
                    s = np.zeros_like(x3[0])
                    for k in range(g.nk):
                        s = s + x3[k]
                    assert bits_equal(interior(g, D[f2], pos), s), (f2, m)


def _boundary_layers_not_both_empty(g, hml, pos):
    """per point of the compute range of pos: a wet cell | a wet face whose two boundary layers are not both empty"""
    hbl = hml.copy(); orc.halo_update(g, hbl, _abi.POS_H)
    ok = np.zeros(g.shape2(pos), dtype=bool)
    for d, f, cL, cR, wet in nc.faces(g):
        if wet and (hbl[cL] > 0. or hbl[cR] > 0.):
            if pos == (_abi.POS_U if d == 0 else _abi.POS_V):
                ok[f] = True
            elif pos == _abi.POS_H:
                ok[cL] = ok[cL] or g.mask2dT[cL] > 0.; ok[cR] = ok[cR] or g.mask2dT[cR] > 0.
    return interior(g, ok, pos)


@pytest.mark.parametrize("name", list(tm.CASES))
def test_every_array_has_something_in_it(name):
    """each expected array is non-zero on at least a quarter of its wet compute-range points (hbd_*: of those whose two boundary layers
    are not both empty) -- a condition on the inputs (seeds, the range of h_ML)"""
    g, I, _, mix, _, _ = tm.expected(name)
    wet = {_abi.POS_H: interior(g, g.mask2dT) > 0., _abi.POS_U: interior(g, g.mask2dCu, _abi.POS_U) > 0.,
           _abi.POS_V: interior(g, g.mask2dCv, _abi.POS_V) > 0.}
    for m in range(NTR):
        for n, a in mix[m].items():
            pos = mc.POS[n]
            pts = wet[pos]
            if n.startswith("hbd"):
                pts = pts & _boundary_layers_not_both_empty(g, I["h_ML"], pos)
            x = interior(g, a, pos)
            nz = (x != 0.0) if x.ndim == 2 else np.any(x != 0.0, axis=0)
            assert pts.sum() > 0 and (nz & pts).sum() >= 0.25 * pts.sum(), (n, m, int((nz & pts).sum()), int(pts.sum()))
            assert not np.any(nz & ~wet[pos]), (n, m)      # dry faces and land: 0


def test_the_record_mirrors_the_header():
    import ctypes as C
    import re
    from pathlib import Path
    text = Path(__file__).resolve().parents[1].joinpath("include", "mom6hip.h").read_text()
    body = re.search(r"typedef struct mom6hip_tracer_mix_diag \{(.*?)\} mom6hip_tracer_mix_diag_t;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\*(\w+)", body)
    assert tuple(fields) == tuple(n for n, _ in _abi.TracerMixDiag._fields_) == mc.NAMES == _abi.ND_MIX_DIAGS + _abi.HBD_MIX_DIAGS
    assert C.sizeof(_abi.TracerMixDiag) == 12 * C.sizeof(C.c_void_p)
    assert all(_abi.MIX_DIAG_KINDS[n][0] == mc.POS[n] for n in mc.NAMES)
