"""The numpy checker of the diagnostics neutral_diffusion and hor_bnd_diffusion post (tests/tracer_mix_checker.py) against the reference's own
modules: MOM_tracer_hor_diff.F90, MOM_neutral_diffusion.F90 and MOM_hor_bnd_diffusion.F90, compiled unmodified under
tests/fortran/tracer_mix_diag_driver.F90 with the diagnostic ids set and a post_data that records what it is given (needs the reference
and amdflang).  The committed stand-in of MOM_diag_mediator posts nothing and stays so: the build helper here compiles a copy of the stub
file in its temporary directory, patched by one line in post_data_2d and one in post_data_3d that call the recorder of the driver, and
asserts that the patch applied.  Compared bitwise on the compute ranges, with the order of the posts, on a closed and on an x-re-entrant
domain: both answer dates x the four coefficient forms, NDIFF_CONTINUOUS = False with PLM and PPM_H4, the boundary diffusion by default,
with HBD_LINEAR_TRANSITION and with APPLY_LIMITER_REMAP, and the boundary diffusion followed by NDIFF_INTERIOR_ONLY neutral diffusion.
One small case is recorded in tests/golden/tracer_mix_diagnostics.json and holds the checker everywhere."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import hbd_checker as hc
import tracer_mix_checker as mc
from helpers import bits_equal, interior
from mom6_amd import _abi
from oracle import orc
from test_reference_kernels import FC, REF, ROOT, STUBS, TRACER_SOURCES

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "tracer_mix_diagnostics.json")
has_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src")) or not os.path.exists(FC), reason="the reference or amdflang is not present")
NTR, DT = 3, 3600.0
PLM, H4 = dict(NDIFF_REMAPPING_SCHEME="PLM"), dict(NDIFF_REMAPPING_SCHEME="PPM_H4")
CASES = {f"nd_{date}_{mode}": dict(date=date, taper=mode in ("taper", "both"), ebt=mode in ("ebt", "both"))
         for date in (20240101, 20240401) for mode in ("plain", "taper", "ebt", "both")}
CASES.update({f"ndd_{date}_{s['NDIFF_REMAPPING_SCHEME'].lower()}": dict(date=date, disc=s) for date in (20240101, 20240401) for s in (PLM, H4)})
CASES.update(hbd_default=dict(hbd={}, neutral=False), hbd_linear=dict(hbd=dict(HBD_LINEAR_TRANSITION=True), neutral=False),
             hbd_limiter_remap=dict(hbd=dict(APPLY_LIMITER_REMAP=True), neutral=False), hbd_then_neutral=dict(hbd={}, date=20240401, interior=True))
GOLDEN_CASE, GOLDEN_GRID = "hbd_then_neutral", dict(ni=10, nj=6, nk=3)


def names_of(kw):
    return (mc.HBD_NAMES if "hbd" in kw else ()) + (mc.ND_NAMES if kw.get("neutral", True) else ())


@functools.lru_cache(maxsize=None)
def state(reentrant_x, ni=14, nj=8, nk=4):
    import test_hor_bnd_diffusion as thbd
    import test_ndiff_taper_ebt as tte
    g, h, tr, h_ML = thbd.case(ni=ni, nj=nj, nk=nk, reentrant=(reentrant_x, False), ntr=2, hml=(0.1, 0.7))
    t = np.ascontiguousarray(np.random.default_rng(31).random(h.shape) * g.mask2dT[None])
    orc.halo_update(g, t, _abi.POS_H)
    return g, h, tr + [t], h_ML, tte.ebt_structure(g, decay=4.0)


def expectation(st, kw, tracers=None):
    """the checker's tracers and arrays (7 outside the compute ranges) for the tracers asked, the order of the posts as ids, the parameters"""
    g, h, tr0, h_ML, ebt_s = st
    tracers = range(NTR) if tracers is None else tracers
    neutral, hbd, disc = kw.get("neutral", True), kw.get("hbd"), kw.get("disc")
    taper, ebt = kw.get("taper", False), kw.get("ebt", False)
    inter = bool(kw.get("interior", False) or taper)
    date = kw.get("date", 20240101)
    KhTr = 5.0e3 if hbd is not None else 800.0
    use_hml = hbd is not None or inter
    tr = [t.copy() for t in tr0]
    names = names_of(kw)
    mix = [({n: np.full(mc.shape_of(g, n), 7.0) for n in names} if m in tracers else None) for m in range(NTR)]
    mc.tracer_hordiff_mix(g, h, DT, tr, KhTr, orc.eos("WRIGHT"), hbd=None if hbd is None else hc.HBDCS(g.H_subroundoff, **hbd), neutral=neutral,
                          disc=disc, h_ML=h_ML if use_hml else None, interior=inter, ebt_struct=ebt_s if ebt else None, mix=mix,
                          NDIFF_ANSWER_DATE=date, NDIFF_TAPERING=taper)
    order = [100 * (m + 1) + mc.NAMES.index(n) + 1 for group in (mc.HBD_NAMES, mc.ND_NAMES) for m in tracers for n in group if n in names]
    params = dict(KHTR=KhTr, KHTR_USE_EBT_STRUCT=ebt, USE_HORIZONTAL_BOUNDARY_DIFFUSION=hbd is not None, USE_NEUTRAL_DIFFUSION=neutral,
                  NDIFF_ANSWER_DATE=date, EQN_OF_STATE="WRIGHT", NDIFF_INTERIOR_ONLY=inter, NDIFF_TAPERING=taper, **(hbd or {}))
    if disc:
        params.update(NDIFF_CONTINUOUS=False, **disc)
    return tr, mix, order, params, use_hml, ebt


def write_case(tmp, st, kw, tracers=None, resident=False, extra=None):
    """the input and parameter files of tracer_mix_diag_driver.F90 (the layout of ebt_tracer_driver's; the last header word carries the ids)"""
    g, h, tr0, h_ML, ebt_s = st
    tracers = range(NTR) if tracers is None else tracers
    tr, mix, order, params, give_hml, use_ebt = expectation(st, kw, tracers)
    bits = sum(1 << mc.NAMES.index(n) for n in names_of(kw)) | sum(1 << (16 + m) for m in tracers)
    zero_h, zero_u, zero_v = g.zeros2(_abi.POS_H), g.zeros2(_abi.POS_U), g.zeros2(_abi.POS_V)
    opt = [NTR, int(use_ebt), 0, 0, int(give_hml), 0, 0, int(use_ebt)]      # use_variable_mixing with the switch, as VarMix_init sets it
    with open(tmp / "in.bin", "wb") as fh:
        np.array([g.ni, g.nj, g.nk, g.halo, int(g.reentrant_x), int(g.reentrant_y), g.first_direction, bits], dtype="<i4").tofile(fh)
        np.array([g.Angstrom_H, g.H_subroundoff, g.dZ_subroundoff, g.H_to_Z, g.Z_to_H, g.g_Earth, g.Rho0, 900.0], dtype="<f8").tofile(fh)
        np.array(opt, dtype="<i4").tofile(fh)
        for n in _abi.ALL_METRICS:
            np.ascontiguousarray(g.metrics[n], dtype="<f8").tofile(fh)
        np.array([DT, 1.0], dtype="<f8").tofile(fh)
        for a in [h, np.zeros(g.shape3(_abi.POS_U)), np.zeros(g.shape3(_abi.POS_V))] + tr0 + [zero_h, zero_u, zero_v, zero_u, zero_v, zero_h, zero_h] + \
                ([h_ML] if give_hml else []) + ([ebt_s] if use_ebt else []):
            np.ascontiguousarray(a, dtype="<f8").tofile(fh)
    with open(tmp / "params.txt", "w") as fh:
        fh.write(f"GPU_RESIDENT_DYNAMICS = {resident}\n")
        for k, v in dict(params, **(extra or {})).items():
            fh.write(f"{k} = {v if isinstance(v, (bool, str, int)) else repr(v)}\n")
    return tr, mix, order


def run(exe, tmp, g):
    """-> (the tracers, [(id, array)] in the order of the posts), or (None, the finished process)"""
    r = subprocess.run([exe, str(tmp / "in.bin"), str(tmp / "out.bin"), str(tmp / "params.txt")], capture_output=True, text=True)
    if r.returncode != 0 or "tracer_mix_diag_driver ok" not in r.stdout:
        return None, r
    tr = np.fromfile(str(tmp / "out.bin"), dtype="<f8").reshape((NTR,) + g.shape3(_abi.POS_H))
    raw = open(str(tmp / "out.bin") + ".posts", "rb").read()
    at, posts = 0, []
    while at < len(raw):
        i, rank, n1, n2, n3 = np.frombuffer(raw, dtype="<i4", count=5, offset=at); at += 20
        a = np.frombuffer(raw, dtype="<f8", count=int(n1) * int(n2) * int(n3), offset=at); at += 8 * a.size
        posts.append((int(i), a.reshape((n2, n1) if rank == 2 else (n3, n2, n1))))
    return tr, posts


def compare(g, tr, posts, want_tr, mix, order, zero_outside=False):
    assert [i for i, _ in posts] == order, ([i for i, _ in posts], order)
    bad = [("tracer", m) for m in range(NTR) if not bits_equal(interior(g, tr[m]), interior(g, want_tr[m]))]
    for i, a in posts:
        m, n = i // 100 - 1, mc.NAMES[i % 100 - 1]
        w = mix[m][n]
        assert a.shape == w.shape, (n, a.shape, w.shape)
        if not bits_equal(interior(g, a, mc.POS[n]), interior(g, w, mc.POS[n])):
            bad.append((n, m))
        if zero_outside:
            rest = a.copy(); sj, si = g.csl(mc.POS[n]); rest[..., sj, si] = 0.0
            if np.any(rest != 0.0):
                bad.append((n, m, "not zero outside the compute range"))
    assert not bad, bad


def patched_stub(tmp):
    """a copy of the stand-ins whose post_data_2d / post_data_3d hand what they are given to the recorder of the driver"""
    text = open(os.path.join(STUBS, "mom6_stubs.F90")).read()
    for rank, call in ((2, "  call mix_record_2d(diag_field_id, field, size(field,1), size(field,2))\n"),
                       (3, "  call mix_record_3d(diag_field_id, field, size(field,1), size(field,2), size(field,3))\n")):
        end = f"end subroutine post_data_{rank}d\n"
        assert text.count(end) == 1, end
        text = text.replace(end, call + end)
    assert text.count("call mix_record_2d(") == 1 and text.count("call mix_record_3d(") == 1
    path = os.path.join(str(tmp), "mom6_stubs.F90")
    open(path, "w").write(text)
    return path


def build(tmp, reference):
    """tracer_mix_diag_driver.F90 on the patched stand-ins and the reference's own tracer modules, or on the module shims and libmom6hip"""
    import test_fortran_abi as fa
    flags = ["-cpp", "-fdefault-real-8", "-O0", "-ffp-contract=off"]
    if reference:
        flags += ["-DREFERENCE_KERNELS", "-DREF_EOS", "-DREF_INTERFACE_HEIGHTS", "-DREF_ALE", f"-I{REF}/config_src/memory/dynamic_symmetric",
                  f"-I{REF}/src/framework", f"-I{REF}/src/equation_of_state", f"-I{REF}/src/ALE"]
        mids = [os.path.join(REF, r) for r in TRACER_SOURCES]
    else:
        mids = [os.path.join(fa.FDIR, s) for s in fa.SHIMS]
    flags += [f"-I{STUBS}", f"-I{tmp}", "-J", str(tmp)]
    objs = []
    for src in [patched_stub(tmp)] + mids + [os.path.join(ROOT, "tests", "fortran", "tracer_mix_diag_driver.F90")]:
        o = os.path.join(str(tmp), os.path.basename(src)[:-4] + ".o")
        r = subprocess.run([FC, *flags, "-c", src, "-o", o], capture_output=True, text=True)
        assert r.returncode == 0, f"{src}:\n" + r.stderr[-3000:]
        objs.append(o)
    exe = os.path.join(str(tmp), "tracer_mix_diag_driver")
    libdir = os.path.join(ROOT, "mom6_amd")
    link = [] if reference else [f"-L{libdir}", "-lmom6hip", f"-Wl,-rpath,{libdir}"]
    r = subprocess.run([FC, *objs, *link, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def ref_exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("tracer_mix_ref"), reference=True)


@has_ref
@pytest.mark.parametrize("reentrant_x", [False, True], ids=["closed", "reentrant_x"])
@pytest.mark.parametrize("name", list(CASES))
def test_reference_equals_the_checker(tmp_path, ref_exe, name, reentrant_x):
    st = state(reentrant_x)
    want_tr, mix, order = write_case(tmp_path, st, CASES[name])
    tr, posts = run(ref_exe, tmp_path, st[0])
    assert tr is not None, (posts.stdout[-300:], posts.stderr[-1500:])
    assert len(order) == NTR * len(names_of(CASES[name]))
    compare(st[0], tr, posts, want_tr, mix, order)
    for i, a in posts:      # the reference's own arrays are not trivial
        if i // 100 == 1:
            assert np.any(interior(st[0], a, mc.POS[mc.NAMES[i % 100 - 1]]) != 0.0), i


@has_ref
def test_reference_with_a_subset_of_the_tracers(tmp_path, ref_exe):
    st = state(True)
    want_tr, mix, order = write_case(tmp_path, st, CASES["hbd_then_neutral"], tracers=(0, 2))
    tr, posts = run(ref_exe, tmp_path, st[0])
    assert tr is not None, posts.stderr[-1500:]
    compare(st[0], tr, posts, want_tr, mix, order)


def _hex(a):
    return [float(x).hex() for x in np.ascontiguousarray(a).ravel()]


def golden_state():
    return state(True, **GOLDEN_GRID)


def test_golden_holds_the_checker():
    """runs everywhere: the recorded posts of the reference's own modules (tracer 0, compute ranges) against the checker, to the bit"""
    gold = json.load(open(GOLDEN))
    st = golden_state()
    g = st[0]
    assert gold["grid"] == [g.ni, g.nj, g.nk] and gold["case"] == GOLDEN_CASE
    _, mix, _, _, _, _ = expectation(st, CASES[GOLDEN_CASE])
    assert set(gold["arrays"]) == set(mc.NAMES)
    for n in mc.NAMES:
        assert _hex(interior(g, mix[0][n], mc.POS[n])) == gold["arrays"][n], n
        assert any(x != "0x0.0p+0" for x in gold["arrays"][n]), n


@has_ref
def test_golden_is_what_the_reference_gives(tmp_path, ref_exe):
    """re-records the golden case from the reference's own modules and compares with the file (MOM6HIP_REGOLD=1 writes it)"""
    st = golden_state()
    g = st[0]
    write_case(tmp_path, st, CASES[GOLDEN_CASE])
    tr, posts = run(ref_exe, tmp_path, g)
    assert tr is not None, posts.stderr[-1500:]
    new = {"grid": [g.ni, g.nj, g.nk], "case": GOLDEN_CASE,
           "source": "the reference's MOM_neutral_diffusion.F90 and MOM_hor_bnd_diffusion.F90 under tests/fortran/tracer_mix_diag_driver.F90, tracer 1",
           "arrays": {mc.NAMES[i % 100 - 1]: _hex(interior(g, a, mc.POS[mc.NAMES[i % 100 - 1]])) for i, a in posts if i // 100 == 1}}
    if os.environ.get("MOM6HIP_REGOLD") == "1":
        with open(GOLDEN, "w") as fh:
            json.dump(new, fh, indent=0, sort_keys=True)
    assert json.load(open(GOLDEN)) == new
