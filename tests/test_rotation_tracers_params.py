"""Quarter-turn reproducibility (tests/rotation.py: the reference's ROTATE_INDEX / .testing `test.rotate` property) of the tracer and
lateral operators: advect_tracer, tracer_hordiff with every one of its branches, thickness_diffuse, mixedlayer_restrat,
horizontal_viscosity on its own, set_viscous_BBL and the vertvisc trio.  For each operator and option set the operator runs on a grid g
and on rotate_grid(g) with turned inputs; the turned-back result has to be the result, value for value, on the compute domain, with the
same iteration counts and statistics.  The turn swaps the x and the y paths of every operator (separate kernel text or separate
launches in the library), the shape (26x18 -> 18x26, 70x22 -> 22x70), first_direction and the topology ((T,F) -> (F,T)), with no second
implementation in between.

On the CPU (no mark) the property is established for the oracle and the Python checkers, option set by option set.  On the GPU the
library is held to (1) parity with the oracle / checker on the TURNED grid, bit for bit, and (2) the turn itself.

Recorded exceptions: option sets that do not turn to the bit on the oracle, because the reference's expression is not symmetric.  Each is
asserted NOT to turn in the entries named, and those entries are left out of the GPU turn assertion:

  * neutral diffusion with NDIFF_ANSWER_DATE = 20240101 (the default): the flux divergences of the four faces of a cell are added into
    one sum in the order east, west, north, south, src/tracer/MOM_neutral_diffusion.F90:837-848 and :882-893; the form of :849-863 and
    :894-908, "(dTracer_N + dTracer_S) + (dTracer_E + dTracer_W)", "recovers rotational symmetry" (NDIFF_ANSWER_DATE > 20240330).  T and S
    still turn; the tracer of zeros and ones does not.
  * epipycnal diffusion (DIFFUSE_ML_TO_INTERIOR) with HOR_DIFF_ANSWER_DATE = 20240101 and HOR_DIFF_LIMIT_BUG (the defaults): the range a
    face limits its tracers to takes the left column's second layer into Tr_La, not Tr_Lb, src/tracer/MOM_tracer_hor_diff.F90:1272-1273
    (u faces) and :1432-1433 (v faces) -- the reference's own "rotational symmetry breaking bug" (:71-73) -- and the fluxes go into one
    tr_flux_conv face after face (:1310-1312, :1320; :1322 keeps tr_flux_E, _W, _N, _S apart with HOR_DIFF_ANSWER_DATE > 20240330).
    T and S turn; the two passive tracers do not.
  * thickness_diffuse with USE_GM_WORK_BUG: the work of the top layer has "the incorrect sign" on the u grid only,
    src/parameterizations/lateral/MOM_thickness_diffuse.F90:1564-1567 against :1601-1603.  Only MEKE%GM_src does not turn.
"""
import functools

import numpy as np
import pytest

import exact_synth as xs
import hbd_checker as hc
import hbd_ebt_checker as hec
import ndiff_checker as nc
import test_epipycnal as tep
import test_hor_bnd_diffusion as thbd
import test_hor_visc as thv
import test_mixedlayer_restrat as tmle
import test_ndiff_taper_ebt as tte
import test_set_viscosity as tsv
import test_thickness_diffuse as ttd
import test_tracer_hor_diff as thd
import test_vert_friction as tvf
from helpers import advect_case, bits_equal, interior
from mom6_amd import _abi
from oracle import orc
from rotation import rot, rot_face, rot_vector, rotate_grid, unrot, unrot_face, unrot_vector

H, U, V = _abi.POS_H, _abi.POS_U, _abi.POS_V
TOPOS = [(True, False), (True, True), (False, False)]
TOPO_IDS = ["reentrant_x", "doubly_reentrant", "closed"]
NI, NJ = 26, 18


# ---- turning a set of named fields ----------------------------------------------------------------------------------------------------
def pos_of(g, a):
    for pos in (H, U, V, _abi.POS_Q):
        if tuple(a.shape[-2:]) == tuple(g.shape2(pos)):
            return pos
    raise ValueError(a.shape)


def dom(g, a):
    return interior(g, a, pos_of(g, a))


def turn(d, vec=(), face=(), back=False):
    """the fields of d in the turned frame (back: from the turned frame): pairs named in vec turn as vectors, pairs named in face as
    face scalars, every other array of two or more dimensions (and every array of a list) as a scalar; the rest is kept"""
    r, rv, rf = (unrot, unrot_vector, unrot_face) if back else (rot, rot_vector, rot_face)
    out = {}
    for pairs, f in ((vec, rv), (face, rf)):
        for a, b in pairs:
            if a in d and d[a] is not None:
                out[a], out[b] = f(d[a], d[b])
    for k, x in d.items():
        if k in out:
            continue
        if isinstance(x, list):
            out[k] = [r(t) for t in x]
        elif isinstance(x, np.ndarray) and x.ndim >= 2:
            out[k] = r(x)
        else:
            out[k] = x
    return out


def differences(g, a, b, equal):
    """the names of the entries of a and b that differ on the compute domain (equal: the comparison of two arrays)"""
    bad = []
    assert set(a) == set(b)
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, list):
            bad += [f"{k}[{m}]" for m, (s, t) in enumerate(zip(x, y)) if not equal(dom(g, s), dom(g, t))]
        elif isinstance(x, np.ndarray) and x.ndim >= 2:
            if not equal(dom(g, x), dom(g, y)):
                bad.append(k)
        elif x is not None and x != y:
            bad.append(k)
    return bad


def turning_differences(op, g, out, out_turned):
    """+0 == -0: a turned zero vector component is -0"""
    return differences(g, out, turn(out_turned, op.VEC, op.FACE, back=True), np.array_equal)


def halo(g, a, pos=H):
    a = np.ascontiguousarray(a)
    orc.halo_update(g, a, pos)
    return a


# ---- the operators: inputs, the oracle (or the checker), the library ------------------------------------------------------------------------
class Dev:
    """device-resident arrays on one DeviceGrid per grid"""

    def __init__(self):
        self.dgs = []

    def dg(self, g):
        from mom6_amd.tracer_advect import DeviceGrid
        self.dgs.append(DeviceGrid(g))
        return self.dgs[-1]

    @staticmethod
    def X(a):
        import torch
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()

    @staticmethod
    def N(a):
        return None if a is None else a.cpu().numpy()

    def close(self):
        for dg in self.dgs:
            dg.close()


class Advect:
    VEC, FACE = (("uhtr", "vhtr"), ("uhr", "vhr")), ()
    SETS = {"PLM": "PLM", "PPM:H3": "PPM:H3", "PPM": "PPM"}
    CU = [0.0, 0.0, 1.0e-7]

    @staticmethod
    def build(ni, nj, topo, nk=4, ntr=3):
        g, c = advect_case(ni=ni, nj=nj, nk=nk, ntr=ntr, hot_frac=0.05, seed=5, cfl=0.1, reentrant_x=topo[0], reentrant_y=topo[1])
        c["tr"][2] = c["tr"][2] * 1.0e-6      # below its conc_underflow in places
        return g, dict(h_end=c["h_end"], uhtr=c["uhtr"], vhtr=c["vhtr"], vol0=c["vol0"], tr=c["tr"])

    @classmethod
    def cu(cls, inp):
        return cls.CU + [0.0] * (len(inp["tr"]) - 3)

    @classmethod
    def oracle(cls, g, inp, scheme):
        tr = [t.copy() for t in inp["tr"]]; vol = inp["vol0"].copy()
        uhr, vhr = g.zeros3(U), g.zeros3(V)
        st = orc.advect_tracer(g, inp["h_end"], inp["uhtr"], inp["vhtr"], 3600.0, 900.0, scheme, tr, conc_underflow=cls.cu(inp), vol_prev=vol,
                               update_vol_prev=True, uhr_out=uhr, vhr_out=vhr)
        return dict(tr=tr, vol=vol, uhr=uhr, vhr=vhr, stats=(st.iterations, st.halo_updates, st.domore_remaining))

    @classmethod
    def hip(cls, dev, dg, g, inp, scheme):
        from mom6_amd.tracer_advect import advect_tracer, tracer_advect_init
        X, N = dev.X, dev.N
        tr = [X(t) for t in inp["tr"]]; vol = X(inp["vol0"]); uhr, vhr = X(g.zeros3(U)), X(g.zeros3(V))
        st = advect_tracer(X(inp["h_end"]), X(inp["uhtr"]), X(inp["vhtr"]), None, 3600.0, dg, tracer_advect_init(900.0, scheme), tr,
                           vol_prev=vol, update_vol_prev=True, uhr_out=uhr, vhr_out=vhr, conc_underflow=cls.cu(inp))
        dg.sync()
        return dict(tr=[N(t) for t in tr], vol=N(vol), uhr=N(uhr), vhr=N(vhr), stats=(st.iterations, st.halo_updates, st.domore_remaining))

    @staticmethod
    def worked(g, inp, out):
        return out["stats"][0] >= 2 and not np.array_equal(dom(g, out["tr"][0]), dom(g, inp["tr"][0])) and np.any(dom(g, out["tr"][2]) == 0.0)


VM_NAMES = dict(KhTr="KHTR", KhTr_Slope_Cff="KHTR_SLOPE_CFF", KhTr_min="KHTR_MIN", KhTr_max="KHTR_MAX", KhTr_passivity_coeff="KHTR_PASSIVITY_COEFF",
                KhTr_passivity_min="KHTR_PASSIVITY_MIN", max_diff_CFL="MAX_TR_DIFFUSION_CFL")


class HorDiff:
    """tracer_hordiff along layers: constant KHTR, and the VarMix / MEKE diffusivities of test_tracer_hor_diff.VM"""
    VEC, FACE = (), (("L2u", "L2v"), ("SN_u", "SN_v"))
    SETS = dict({"khtr": dict(KhTr=50.0, use=()), "khtr_cfl_itts": dict(KhTr=5.0e7, check=True, use=())}, **{f"varmix_{n}": v for n, v in thd.VM.items()})

    @staticmethod
    def build(ni, nj, topo, nk=4, ntr=3):
        g, h, tr = thd.case(ni, nj, nk, reentrant=topo)
        rng = np.random.default_rng(31)
        tr = tr + [halo(g, rng.random(h.shape) * g.mask2dT[None]) for _ in range(ntr - len(tr))]
        return g, dict(h=h, tr=tr, **thd.varmix_fields(g))

    @staticmethod
    def oracle(g, inp, opt):
        kw = dict(opt); use = kw.pop("use"); meke = kw.pop("meke", None); check = kw.pop("check", False)
        tr = [t.copy() for t in inp["tr"]]
        st = orc.tracer_hordiff(g, inp["h"], 3600.0, tr, kw.pop("KhTr"), check_diffusive_CFL=check, VarMix={n: inp[n] for n in use} if use else None,
                                MEKE=None if meke is None else dict(Kh=inp["Kh"], KhTr_fac=meke), **kw)
        return dict(tr=tr, stats=(st.num_itts, st.halo_updates, st.max_CFL))

    @staticmethod
    def hip(dev, dg, g, inp, opt):
        from mom6_amd.tracer_hor_diff import tracer_hor_diff_init, tracer_hordiff
        X, N = dev.X, dev.N
        meke = opt.get("meke")
        CS = tracer_hor_diff_init(CHECK_DIFFUSIVE_CFL=opt.get("check", False), **{VM_NAMES[k]: v for k, v in opt.items() if k in VM_NAMES})
        tr = [X(t) for t in inp["tr"]]
        st = tracer_hordiff(X(inp["h"]), 3600.0, None if meke is None else dict(Kh=X(inp["Kh"]), KhTr_fac=meke),
                            {n: X(inp[n]) for n in opt["use"]} if opt["use"] else None, None, dg, CS, tr)
        dg.sync()
        return dict(tr=[N(t) for t in tr], stats=(st.num_itts, st.halo_updates, st.max_CFL))

    @staticmethod
    def worked(g, inp, out):
        return not np.array_equal(dom(g, out["tr"][0]), dom(g, inp["tr"][0]))


class Neutral:
    """USE_NEUTRAL_DIFFUSION through the oracle, with NDIFF_ANSWER_DATE = 20240401 but for the recorded exception"""
    VEC, FACE = (), ()
    SETS = {
        "wright": dict(KhTr=800.0), "linear_ref_pres": dict(KhTr=800.0, ref_pres=2.0e7, eos="LINEAR"), "interior": dict(KhTr=800.0, interior=True),
        "itts": dict(KhTr=1.0e9, max_diff_CFL=2.5), "itts_recalc_linear": dict(KhTr=1.0e9, max_diff_CFL=2.5, recalc_neutral_surf=True, eos="LINEAR"),
        "itts_recalc_interior": dict(KhTr=1.0e9, max_diff_CFL=2.5, recalc_neutral_surf=True, interior=True), "p_surf": dict(KhTr=800.0, p_surf=True),
        "legacy_20240101": dict(KhTr=800.0, date=20240101),
    }

    @staticmethod
    def build(ni, nj, topo, nk=6, ntr=3):
        g, h, tr = tte.nd_case(ntr=ntr, ni=ni, nj=nj, nk=nk, reentrant=topo)
        return g, dict(h=h, tr=tr, h_ML=tte.boundary_layer(g, h, 0.3), p_surf=np.ascontiguousarray(1.0e4 * np.random.default_rng(8).random(g.shape2(H))))

    @staticmethod
    def oracle(g, inp, opt):
        tr = [t.copy() for t in inp["tr"]]
        nd = dict(eos=orc.eos(opt.get("eos", "WRIGHT")), idx_T=0, idx_S=1, ndiff_answer_date=opt.get("date", 20240401), h_ML=inp["h_ML"] if opt.get("interior") else None,
                  p_surf=inp["p_surf"] if opt.get("p_surf") else None, **{k: opt[k] for k in ("ref_pres", "recalc_neutral_surf") if k in opt})
        st = orc.tracer_hordiff(g, inp["h"], 3600.0, tr, opt["KhTr"], max_diff_CFL=opt.get("max_diff_CFL", -1.0), neutral=nd)
        return dict(tr=tr, stats=(st.num_itts, st.halo_updates, st.max_CFL))

    @staticmethod
    def hip(dev, dg, g, inp, opt):
        from mom6_amd.tracer_hor_diff import tracer_hor_diff_init, tracer_hordiff
        X, N = dev.X, dev.N
        CS = tracer_hor_diff_init(KHTR=opt["KhTr"], MAX_TR_DIFFUSION_CFL=opt.get("max_diff_CFL", -1.0), USE_NEUTRAL_DIFFUSION=True,
                                  NDIFF_REF_PRES=opt.get("ref_pres", -1.0), NDIFF_ANSWER_DATE=opt.get("date", 20240401),
                                  RECALC_NEUTRAL_SURF=opt.get("recalc_neutral_surf", False), NDIFF_INTERIOR_ONLY=bool(opt.get("interior")))
        tr = [X(t) for t in inp["tr"]]
        tv = dict(T=tr[0], S=tr[1], eqn_of_state=orc.eos(opt.get("eos", "WRIGHT")), p_surf=X(inp["p_surf"]) if opt.get("p_surf") else None)
        st = tracer_hordiff(X(inp["h"]), 3600.0, None, None, dict(h_ML=X(inp["h_ML"])) if opt.get("interior") else None, dg, CS, tr, tv=tv)
        dg.sync()
        return dict(tr=[N(t) for t in tr], stats=(st.num_itts, st.halo_updates, st.max_CFL))

    worked = HorDiff.worked


class TaperEBT:
    """NDIFF_TAPERING / KHTR_USE_EBT_STRUCT through tests/ndiff_checker.py (NDIFF_ANSWER_DATE = 20240401)"""
    VEC, FACE = (), ()
    SETS = {"none": dict(), "taper": dict(taper=True), "ebt": dict(ebt=True), "both": dict(taper=True, ebt=True),
            "both_itts_recalc": dict(taper=True, ebt=True, KhTr=1.0e9, max_diff_CFL=2.5, recalc=True)}

    @staticmethod
    def build(ni, nj, topo, nk=6, ntr=3):
        g, h, tr = tte.nd_case(ntr=ntr, ni=ni, nj=nj, nk=nk, reentrant=topo)
        return g, dict(h=h, tr=tr, h_ML=tte.boundary_layer(g, h), ebt=tte.ebt_structure(g))

    @staticmethod
    def oracle(g, inp, opt):
        tr = [t.copy() for t in inp["tr"]]
        st = nc.tracer_hordiff_neutral(g, inp["h"], 3600.0, tr, opt.get("KhTr", 800.0), orc.eos("WRIGHT"), max_diff_CFL=opt.get("max_diff_CFL", -1.0),
                                       h_ML=inp["h_ML"], ebt_struct=inp["ebt"] if opt.get("ebt") else None, recalc_neutral_surf=opt.get("recalc", False),
                                       NDIFF_TAPERING=opt.get("taper", False), NDIFF_ANSWER_DATE=20240401)
        return dict(tr=tr, stats=tuple(st))

    @staticmethod
    def hip(dev, dg, g, inp, opt):
        from mom6_amd.tracer_hor_diff import tracer_hor_diff_init, tracer_hordiff
        X, N = dev.X, dev.N
        CS = tracer_hor_diff_init(KHTR=opt.get("KhTr", 800.0), MAX_TR_DIFFUSION_CFL=opt.get("max_diff_CFL", -1.0), USE_NEUTRAL_DIFFUSION=True,
                                  NDIFF_ANSWER_DATE=20240401, RECALC_NEUTRAL_SURF=opt.get("recalc", False), NDIFF_INTERIOR_ONLY=True,
                                  NDIFF_TAPERING=opt.get("taper", False), KHTR_USE_EBT_STRUCT=bool(opt.get("ebt")))
        tr = [X(t) for t in inp["tr"]]
        tv = dict(T=tr[0], S=tr[1], eqn_of_state=orc.eos("WRIGHT"), p_surf=None)
        st = tracer_hordiff(X(inp["h"]), 3600.0, None, dict(ebt_struct=X(inp["ebt"])) if opt.get("ebt") else None, dict(h_ML=X(inp["h_ML"])), dg, CS, tr, tv=tv)
        dg.sync()
        return dict(tr=[N(t) for t in tr], stats=(st.num_itts, st.halo_updates, st.max_CFL))

    worked = HorDiff.worked


class HBD:
    """USE_HORIZONTAL_BOUNDARY_DIFFUSION: tests/hbd_checker.py (with ebt: tests/hbd_ebt_checker.py), then the along-layer branch of the oracle"""
    VEC, FACE = (), ()
    SETS = {"default": dict(), "linear": dict(hbd=dict(HBD_LINEAR_TRANSITION=True)), "ppm_h4_extrap": dict(hbd=dict(HBD_REMAPPING_SCHEME="PPM_H4", HBD_BOUNDARY_EXTRAP=True)),
            "cfl_itts": dict(KhTr=6.0e7, check=True), "ebt": dict(ebt=True), "ebt_khtr_min_full_depth": dict(ebt=True, KhTr_min=2.0e3, dt=5.0, full=True)}

    @staticmethod
    def build(ni, nj, topo, nk=6, ntr=2):
        g, h, tr, h_ML = thbd.case(ni, nj, nk, reentrant=topo, ntr=ntr)
        return g, dict(h=h, tr=tr, h_ML=h_ML, ebt=tte.ebt_structure(g, decay=4.0))

    @staticmethod
    def oracle(g, inp, opt):
        tr = [t.copy() for t in inp["tr"]]
        KhTr, check, dt, CS = opt.get("KhTr", 5.0e3), opt.get("check", False), opt.get("dt", 3600.0), hc.HBDCS(g.H_subroundoff, **opt.get("hbd", {}))
        if opt.get("ebt"):
            n = hec.tracer_hordiff_hbd(g, inp["h"], dt, tr, KhTr, inp["h_ML"], CS, inp["ebt"], KhTr_min=opt.get("KhTr_min", 0.0), FULL_DEPTH_KHTR_MIN=opt.get("full", False))
            KhTr = max(KhTr, opt.get("KhTr_min", 0.0))
        else:
            n = hc.tracer_hordiff_hbd(g, inp["h"], dt, tr, KhTr, inp["h_ML"], CS, check_diffusive_CFL=check)
        st = orc.tracer_hordiff(g, inp["h"], dt, tr, KhTr, check_diffusive_CFL=check)
        return dict(tr=tr, stats=(st.num_itts, st.halo_updates + n, st.max_CFL))

    @staticmethod
    def hip(dev, dg, g, inp, opt):
        from mom6_amd.tracer_hor_diff import tracer_hor_diff_init, tracer_hordiff
        X, N = dev.X, dev.N
        kw = dict(KHTR=opt.get("KhTr", 5.0e3), CHECK_DIFFUSIVE_CFL=opt.get("check", False), USE_HORIZONTAL_BOUNDARY_DIFFUSION=True, **opt.get("hbd", {}))
        if opt.get("ebt"):
            kw.update(KHTR_MIN=opt.get("KhTr_min", 0.0), FULL_DEPTH_KHTR_MIN=opt.get("full", False), KHTR_USE_EBT_STRUCT=True)
        tr = [X(t) for t in inp["tr"]]
        st = tracer_hordiff(X(inp["h"]), opt.get("dt", 3600.0), None, dict(ebt_struct=X(inp["ebt"])) if opt.get("ebt") else None, dict(h_ML=X(inp["h_ML"])), dg,
                            tracer_hor_diff_init(**kw), tr)
        dg.sync()
        return dict(tr=[N(t) for t in tr], stats=(st.num_itts, st.halo_updates, st.max_CFL))

    worked = HorDiff.worked


class Epipycnal:
    """DIFFUSE_ML_TO_INTERIOR through the oracle"""
    VEC, FACE = (), ()
    SETS = {"20240401": dict(answer_date=20240401), "20240401_exact": dict(answer_date=20240401, exact=True),
            "20240401_no_limit_bug_ml_scale": dict(answer_date=20240401, limit_bug=False, ML_KhTr_scale=0.4),
            "20240401_cfl_itts": dict(answer_date=20240401, KhTr=2.0e5, check=True, dt=86400.0 * 5), "legacy_20240101": dict()}
    NAMES = {"ML_KhTr_scale": "ML_KHTR_SCALE", "answer_date": "HOR_DIFF_ANSWER_DATE", "limit_bug": "HOR_DIFF_LIMIT_BUG"}

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def build(ni, nj, topo, nk=9, exact=False):
        g, h, tr, eos, Rlay = tep.layered_case(ni, nj, nk, reentrant=topo, exact=exact)
        return g, dict(h=h, tr=tr, eos=eos, Rlay=Rlay)

    @classmethod
    def oracle(cls, g, inp, opt):
        tr = [t.copy() for t in inp["tr"]]
        st = orc.tracer_hordiff(g, inp["h"], opt.get("dt", 86400.0), tr, opt.get("KhTr", 800.0), check_diffusive_CFL=opt.get("check", False),
                                epipycnal=tep.epi(inp["eos"], inp["Rlay"], **{k: v for k, v in opt.items() if k in cls.NAMES}))
        return dict(tr=tr, stats=(st.num_itts, st.halo_updates, st.max_CFL))

    @classmethod
    def hip(cls, dev, dg, g, inp, opt):
        from mom6_amd.tracer_hor_diff import tracer_hor_diff_init, tracer_hordiff
        X, N = dev.X, dev.N
        CS = tracer_hor_diff_init(KHTR=opt.get("KhTr", 800.0), CHECK_DIFFUSIVE_CFL=opt.get("check", False), DIFFUSE_ML_TO_INTERIOR=True,
                                  **{cls.NAMES[k]: v for k, v in opt.items() if k in cls.NAMES})
        tr = [X(t) for t in inp["tr"]]
        st = tracer_hordiff(X(inp["h"]), opt.get("dt", 86400.0), None, None, None, dg, CS, tr, tv=dict(T=tr[0], S=tr[1], eqn_of_state=inp["eos"], P_Ref=2.0e7),
                            GV=dict(Rlay=inp["Rlay"], nkml=tep.NKML, nk_rho_varies=tep.NKMB))
        dg.sync()
        return dict(tr=[N(t) for t in tr], stats=(st.num_itts, st.halo_updates, st.max_CFL))

    @staticmethod
    def worked(g, inp, out):
        return not np.array_equal(dom(g, out["tr"][2]), dom(g, inp["tr"][2]))


class ThicknessDiffuse:
    VEC = (("uhtr", "vhtr"), ("uhGM", "vhGM"), ("slope_x", "slope_y"), ("u", "v"))
    FACE = (("L2u", "L2v"), ("SN_u", "SN_v"), ("Res_fn_u", "Res_fn_v"), ("Depth_fn_u", "Depth_fn_v"))
    SETS = ttd.VARIANTS

    @staticmethod
    def build(ni, nj, topo, nk=6):
        g, d = ttd.case(ni, nj, nk, reentrant_x=topo[0], reentrant_y=topo[1])
        return g, dict(d, **ttd.fields(g))

    @staticmethod
    def args(g, inp, opt):
        kw = dict(opt); eos = kw.pop("eos", "WRIGHT"); use = kw.pop("use", ()); work = kw.pop("work", False)
        args = {n: inp[n] for n in use}
        if work:
            args["MEKE_GM_src"] = np.full(g.shape2(H), 7.0)
        if eos is None:      # (as test_thickness_diffuse.run_oracle sets them)
            args["Rlay"] = 1025.0 + 0.5 * np.arange(g.nk)
            if kw.get("use_FGNV_streamfn"):
                gp = np.zeros(g.nk + 1); gp[0] = g.g_Earth; gp[1:g.nk] = (g.g_Earth / g.Rho0) * np.diff(args["Rlay"])
                args["g_prime"] = gp
        return kw, args, eos

    @classmethod
    def oracle(cls, g, inp, opt):
        kw, args, eos = cls.args(g, inp, opt)
        cs = orc.thickness_diffuse_cs(g, **kw, **args)
        out = dict(h=inp["h"].copy(), uhtr=np.zeros_like(inp["u"]), vhtr=np.zeros_like(inp["v"]), uhGM=np.zeros_like(inp["u"]), vhGM=np.zeros_like(inp["v"]))
        orc.thickness_diffuse(g, cs, out["h"], out["uhtr"], out["vhtr"], inp["T"], inp["S"], None if eos is None else orc.eos(eos), ttd.DT, out["uhGM"], out["vhGM"])
        out["GM_src"] = cs._keep.get("MEKE_GM_src")
        return out

    @classmethod
    def hip(cls, dev, dg, g, inp, opt):
        from mom6_amd.pressure_force import EOS_init
        from mom6_amd.thickness_diffuse import thickness_diffuse, thickness_diffuse_init
        X, N = dev.X, dev.N
        kw, args, eos = cls.args(g, inp, opt)
        CS = thickness_diffuse_init(dg, THICKNESSDIFFUSE=True, **{ttd.REF[k]: v for k, v in kw.items() if k in ttd.REF})
        h, uhtr, vhtr = X(inp["h"]), X(np.zeros_like(inp["u"])), X(np.zeros_like(inp["v"]))
        cdp = dict(uhGM=X(np.zeros_like(inp["u"])), vhGM=X(np.zeros_like(inp["v"])))
        meke = {n: args[n] for n in ("Rlay", "g_prime") if n in args}
        if "MEKE_Kh" in args:
            meke["Kh"] = X(args["MEKE_Kh"])
        if "MEKE_GM_src" in args:
            meke["GM_src"] = X(args["MEKE_GM_src"])
        vm = {n: X(a) for n, a in args.items() if n in ("L2u", "L2v", "SN_u", "SN_v", "Res_fn_u", "Res_fn_v", "slope_x", "slope_y", "cg1", "Depth_fn_u", "Depth_fn_v")}
        thickness_diffuse(h, uhtr, vhtr, None if eos is None else (X(inp["T"]), X(inp["S"]), EOS_init(eos)), ttd.DT, dg, meke,
                          vm if kw.get("use_variable_mixing") else None, cdp, CS)
        dg.sync()
        return dict(h=N(h), uhtr=N(uhtr), vhtr=N(vhtr), uhGM=N(cdp["uhGM"]), vhGM=N(cdp["vhGM"]), GM_src=N(meke.get("GM_src")))

    @staticmethod
    def worked(g, inp, out):
        return not np.array_equal(dom(g, out["h"]), dom(g, inp["h"])) and np.abs(dom(g, out["uhGM"])).max() > 0 and np.abs(dom(g, out["vhGM"])).max() > 0 \
            and (out["GM_src"] is None or not np.all(dom(g, out["GM_src"]) == 7.0))


class Restrat:
    VEC, FACE = (("uhtr", "vhtr"), ("uhml", "vhml"), ("u", "v")), ()
    SETS = tmle.VARIANTS

    @staticmethod
    def build(ni, nj, topo, nk=8):
        g, d = tmle.case(ni, nj, nk, reentrant_x=topo[0], reentrant_y=topo[1])
        return g, dict(d, **tmle.fields(g, d))

    @staticmethod
    def args(opt):
        kw = dict(opt)
        return kw, tuple(kw.pop("use", ())) + tuple(kw.pop("also", ()))

    @classmethod
    def oracle(cls, g, inp, opt):
        kw, use = cls.args(opt)
        state = {n: inp[n].copy() for n in use}
        cs = orc.mixedlayer_restrat_cs(g, **kw, **state)
        out = dict(h=inp["h"].copy(), uhtr=np.zeros_like(inp["u"]), vhtr=np.zeros_like(inp["v"]), uhml=np.zeros_like(inp["u"]), vhml=np.zeros_like(inp["v"]))
        orc.mixedlayer_restrat(g, cs, out["h"], out["uhtr"], out["vhtr"], inp["T"], inp["S"], orc.eos("WRIGHT"), inp["ustar"], tmle.DT,
                               inp["h_MLD"] if kw.get("MLE_use_PBL_MLD") else None, out["uhml"], out["vhml"])
        out.update({n: state[n] for n in use if n.startswith("MLD_filtered")})
        return out

    @classmethod
    def hip(cls, dev, dg, g, inp, opt):
        from mom6_amd.mixedlayer_restrat import mixedlayer_restrat, mixedlayer_restrat_init
        from mom6_amd.pressure_force import EOS_init
        X, N = dev.X, dev.N
        kw, use = cls.args(opt)
        state = {n: X(inp[n]) for n in use if n.startswith("MLD_filtered")}
        CS = mixedlayer_restrat_init(dg, **{tmle.REF[k]: v for k, v in kw.items()}, **state)
        o = dict(h=X(inp["h"]), uhtr=X(np.zeros_like(inp["u"])), vhtr=X(np.zeros_like(inp["v"])), uhml=X(np.zeros_like(inp["u"])), vhml=X(np.zeros_like(inp["v"])))
        mixedlayer_restrat(o["h"], o["uhtr"], o["vhtr"], (X(inp["T"]), X(inp["S"]), EOS_init("WRIGHT")), dict(ustar=X(inp["ustar"])), tmle.DT, None,
                           X(inp["h_MLD"]) if kw.get("MLE_use_PBL_MLD") else None, None, dict(Rd_dx_h=X(inp["Rd_dx_h"])) if "Rd_dx_h" in use else None,
                           dg, CS, o["uhml"], o["vhml"])
        dg.sync()
        return {n: N(a) for n, a in dict(o, **state).items()}

    @staticmethod
    def worked(g, inp, out):
        return not np.array_equal(dom(g, out["h"]), dom(g, inp["h"])) and max(np.abs(dom(g, out["uhml"])).max(), np.abs(dom(g, out["vhml"])).max()) > 0 \
            and all(not np.array_equal(dom(g, out[n]), dom(g, inp[n])) for n in out if n.startswith("MLD_filtered"))


class HorVisc:
    """horizontal_viscosity alone: test_hor_visc.VARIANTS and the MEKE sets"""
    VEC, FACE = (("u", "v"), ("diffu", "diffv")), (("hu_cont", "hv_cont"),)
    SETS = dict({n: dict(kw=kw, meke=()) for n, kw in thv.VARIANTS.items()}, **{f"meke_{n}": dict(kw=kw, meke=m) for n, (kw, m) in thv.MEKE_VARIANTS.items()})
    UNCHECKED = ("biharmonic_default", "cont_thickness")      # zeros by construction; never run on the CPU before: no "did something" assertion

    @staticmethod
    def build(ni, nj, topo, nk=3):
        g, d = thv.case(ni, nj, nk, reentrant_x=topo[0], reentrant_y=topo[1])
        hu = np.zeros_like(d["u"]); hu[:, :, 1:-1] = 0.5 * (d["h"][:, :, :-1] + d["h"][:, :, 1:]) * 1.01
        hv = np.zeros_like(d["v"]); hv[:, 1:-1, :] = 0.5 * (d["h"][:, :-1, :] + d["h"][:, 1:, :]) * 1.01
        Ku, Au, src = thv.meke_fields(g)
        return g, dict(d, hu_cont=hu, hv_cont=hv, Ku=Ku, Au=Au, mom_src=src)

    @staticmethod
    def oracle(g, inp, opt):
        kw = opt["kw"]
        cs = orc.hor_visc_cs(g, thv.DT, **kw)
        src = orc.hor_visc_set_meke(cs, **{n: inp[n].copy() for n in opt["meke"]}) if opt["meke"] else None
        cont = dict(hu_cont=inp["hu_cont"], hv_cont=inp["hv_cont"]) if kw.get("use_cont_thick") else {}
        du, dv = orc.horizontal_viscosity(g, cs, inp["u"], inp["v"], inp["h"], thv.DT, **cont)
        return dict(diffu=du, diffv=dv, mom_src=src)

    @staticmethod
    def hip(dev, dg, g, inp, opt):
        from mom6_amd.hor_visc import hor_visc_init, horizontal_viscosity
        X, N = dev.X, dev.N
        kw = opt["kw"]
        CS = hor_visc_init(dg, thv.DT, device_arrays=True, **(dict(USE_MEKE=True) if opt["meke"] else {}), **{thv.REF_NAMES[k]: v for k, v in kw.items()})
        du, dv = X(np.zeros_like(inp["u"])), X(np.zeros_like(inp["v"]))
        M = {n: X(inp[n]) for n in opt["meke"]} if opt["meke"] else None
        cont = dict(hu_cont=X(inp["hu_cont"]), hv_cont=X(inp["hv_cont"])) if kw.get("use_cont_thick") else {}
        horizontal_viscosity(X(inp["u"]), X(inp["v"]), X(inp["h"]), du, dv, M, None, dg, CS, **cont)
        dg.sync()
        return dict(diffu=N(du), diffv=N(dv), mom_src=N(M["mom_src"]) if M and "mom_src" in M else None)

    @staticmethod
    def worked(g, inp, out):
        return np.abs(dom(g, out["diffu"])).max() > 0 and np.abs(dom(g, out["diffv"])).max() > 0 and (out["mom_src"] is None or not np.all(dom(g, out["mom_src"]) == -7.0))


BBL_OUT = ("Kv_bbl_u", "Kv_bbl_v", "bbl_thick_u", "bbl_thick_v", "Ray_u", "Ray_v")


class SetViscousBBL:
    VEC, FACE = (("u", "v"),), (("Kv_bbl_u", "Kv_bbl_v"), ("bbl_thick_u", "bbl_thick_v"), ("Ray_u", "Ray_v"))
    SETS = tsv.VARIANTS

    @staticmethod
    def build(ni, nj, topo, nk=8):
        g = xs.make_grid(ni, nj, nk, reentrant_x=topo[0], reentrant_y=topo[1])
        return g, xs.make_state(g, umax=0.3)

    @staticmethod
    def oracle(g, inp, opt):
        a = tsv.run_oracle(g, inp, **opt)
        return {n: a[n] for n in BBL_OUT}

    @staticmethod
    def hip(dev, dg, g, inp, opt):
        from mom6_amd.pressure_force import EOS_init
        from mom6_amd.set_viscosity import set_visc_init, set_viscous_BBL
        from mom6_amd.vert_friction import vertvisc_type
        X, N = dev.X, dev.N
        pk = {tsv.REF[k]: v for k, v in opt.items()}
        if not opt.get("BBL_use_EOS", True):
            pk["Rlay"] = tsv.rlay(g.nk)
        arrs = {n: X(a) for n, a in tsv.visc_arrays(g, inp).items()}
        set_viscous_BBL(X(inp["u"]), X(inp["v"]), X(inp["h"]), (X(inp["T"]), X(inp["S"]), EOS_init("WRIGHT")), vertvisc_type(**arrs), dg,
                        set_visc_init(dg, HBBL=10.0, KV=1.0e-4, **pk))
        dg.sync()
        return {n: N(arrs[n]) for n in BBL_OUT}

    @staticmethod
    def worked(g, inp, out):
        return all(np.abs(dom(g, out[n])).max() > 0 for n in BBL_OUT[:4])


class VertVisc:
    """vertvisc_coef, vertvisc_remnant and vertvisc: column operators whose u-point and v-point halves are separate launches"""
    VEC = (("u", "v"), ("taux", "tauy"), ("taux_bot", "tauy_bot"))
    FACE = (("Kv_bbl_u", "Kv_bbl_v"), ("bbl_thick_u", "bbl_thick_v"), ("Ray_u", "Ray_v"), ("nkml_visc_u", "nkml_visc_v"), ("a_u", "a_v"), ("h_u", "h_v"),
            ("visc_rem_u", "visc_rem_v"))
    SETS = {f"v{n}_" + ("_".join(kw) or "default"): kw for n, kw in enumerate(tvf.VARIANTS)}
    ARRS = ("Kv_bbl_u", "Kv_bbl_v", "bbl_thick_u", "bbl_thick_v", "Ray_u", "Ray_v", "nkml_visc_u", "nkml_visc_v", "Kv_shear", "ustar")
    NAMES = dict(harmonic_visc="HARMONIC_VISC", harm_BL_val="HARMONIC_BL_SCALE", Kvml_invZ2="KV_ML_INVZ2", Hmix="HMIX_FIXED", bottomdraglaw="BOTTOMDRAGLAW",
                 Kv_extra_bbl="KV_EXTRA_BBL", direct_stress="DIRECT_STRESS", CFL_based_trunc="CFL_BASED_TRUNCATIONS", maxvel="MAXVEL",
                 vel_underflow="VEL_UNDERFLOW", dynamic_viscous_ML="DYNAMIC_VISCOUS_ML", nkml="NKML", CFL_trunc="CFL_TRUNCATE")
    DT = 900.0

    @staticmethod
    def build(ni, nj, topo, nk=7):
        g, st, arrs, taux, tauy = tvf.vv_case(ni, nj, nk, with_shear=True, with_ray=True, with_ml=True, reentrant_x=topo[0], reentrant_y=topo[1])
        return g, dict(u=st["u"], v=st["v"], h=st["h"], taux=taux, tauy=tauy, **arrs)

    @classmethod
    def arrs(cls, inp, opt):
        ml = bool(opt.get("dynamic_viscous_ML") or opt.get("nkml"))
        return {n: inp[n] for n in cls.ARRS if ml or n not in ("nkml_visc_u", "nkml_visc_v", "ustar")}

    @classmethod
    def oracle(cls, g, inp, opt):
        cs = orc.vertvisc_cs(g, Kv=1.0e-4, Hbbl=10.0, **opt)
        visc = orc.vertvisc_type(**cls.arrs(inp, opt))
        orc.vertvisc_coef(g, cs, inp["u"], inp["v"], inp["h"], visc, cls.DT)
        o = dict(visc_rem_u=g.zeros3(U), visc_rem_v=g.zeros3(V), u=inp["u"].copy(), v=inp["v"].copy(), taux_bot=g.zeros2(U), tauy_bot=g.zeros2(V))
        orc.vertvisc_remnant(g, cs, visc, o["visc_rem_u"], o["visc_rem_v"], cls.DT)
        orc.vertvisc(g, cs, o["u"], o["v"], inp["h"], inp["taux"], inp["tauy"], visc, cls.DT, o["taux_bot"], o["tauy_bot"])
        return dict(o, ntrunc=int(cs.ntrunc), **{n: cs._arrs[n] for n in ("a_u", "a_v", "h_u", "h_v")})

    @classmethod
    def hip(cls, dev, dg, g, inp, opt):
        from mom6_amd.vert_friction import vertvisc, vertvisc_coef, vertvisc_init, vertvisc_ntrunc, vertvisc_remnant, vertvisc_type
        X, N = dev.X, dev.N
        CS = vertvisc_init(dg, device_arrays=True, KV=1.0e-4, HBBL=10.0, **{cls.NAMES[k]: v for k, v in opt.items()})
        visc = vertvisc_type(**{n: X(a) for n, a in cls.arrs(inp, opt).items()})
        o = dict(visc_rem_u=X(g.zeros3(U)), visc_rem_v=X(g.zeros3(V)), u=X(inp["u"]), v=X(inp["v"]), taux_bot=X(g.zeros2(U)), tauy_bot=X(g.zeros2(V)))
        h = X(inp["h"])
        vertvisc_coef(o["u"], o["v"], h, None, None, visc, None, cls.DT, dg, CS)
        vertvisc_remnant(visc, o["visc_rem_u"], o["visc_rem_v"], cls.DT, dg, CS)
        vertvisc(o["u"], o["v"], h, (X(inp["taux"]), X(inp["tauy"])), visc, cls.DT, None, None, None, dg, CS, o["taux_bot"], o["tauy_bot"])
        dg.sync()
        return dict({n: N(a) for n, a in o.items()}, ntrunc=int(vertvisc_ntrunc(dg, CS)), **{n: N(CS.arrays[n]) for n in ("a_u", "a_v", "h_u", "h_v")})

    @staticmethod
    def worked(g, inp, out):
        return not np.array_equal(dom(g, out["u"]), dom(g, inp["u"])) and not np.array_equal(dom(g, out["v"]), dom(g, inp["v"])) \
            and np.abs(dom(g, out["a_u"])).max() > 0 and np.abs(dom(g, out["visc_rem_v"])).max() > 0


OPS = dict(advect=Advect, hordiff=HorDiff, neutral=Neutral, taper_ebt=TaperEBT, hbd=HBD, epipycnal=Epipycnal, thickness_diffuse=ThicknessDiffuse,
           restrat=Restrat, hor_visc=HorVisc, set_viscous_BBL=SetViscousBBL, vertvisc=VertVisc)
# the option sets that do not turn on the oracle and the entries of their results that do not (the docstring gives the reference's lines): at most
# the neutral-diffusion legacy date and two more
EXCEPTIONS = {("neutral", "legacy_20240101"): {"tr[2]"}, ("epipycnal", "legacy_20240101"): {"tr[2]", "tr[3]"},
              ("thickness_diffuse", "stored_slopes_work"): {"GM_src"}}
assert len(EXCEPTIONS) <= 3
# (which tracers the epipycnal limit bug reaches depends on the grid: at 70x22 T does not turn either; on the GPU none of its tracers is held to the turn)
GPU_EXCEPTIONS = {**EXCEPTIONS, ("epipycnal", "legacy_20240101"): {f"tr[{m}]" for m in range(4)}}


def build(op, ni, nj, topo, size, opt):
    if op is Epipycnal:
        return op.build(ni, nj, topo, exact=bool(opt.get("exact")), **size)
    return op.build(ni, nj, topo, **size)


# ---- the face-scalar helper against the reference's own rotation (oracle/_ref; only where it was built) ------------------------------------
def test_face_scalar_turn_is_the_reference_rotation():
    """rot_face is rotate_array_pair of src/framework/MOM_array_transform.F90 with turns = -1: each member is rotate_array of the other
    (compiled unmodified into oracle/_ref), no sign; unrot_face is the turn back"""
    import ctypes as C
    R = orc.ref_lib()
    if R is None or not hasattr(R, "ref_rotate_array"):
        pytest.skip("oracle/_ref not built (the reference sources only exist in the build container)")
    P = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))

    def ref_rot(a, turns):
        a = np.ascontiguousarray(a)
        k, n, m = a.shape
        out = np.zeros((k, m, n) if turns % 2 else (k, n, m))
        R.ref_rotate_array(m, n, k, P(a), turns, P(out))
        return out

    rng = np.random.default_rng(11)
    nk, nj, ni = 3, 7, 11
    au = rng.standard_normal((nk, nj, ni + 1)); av = rng.standard_normal((nk, nj + 1, ni))
    ru, rv = rot_face(au, av)
    assert ru.shape == (nk, ni, nj + 1) and rv.shape == (nk, ni + 1, nj)      # a v-point array of the original is a u-point array of the turn
    assert np.array_equal(ru, ref_rot(av, -1)) and np.array_equal(rv, ref_rot(au, -1))
    bu, bv = unrot_face(ru, rv)
    assert np.array_equal(bu, au) and np.array_equal(bv, av)
    assert np.array_equal(bu, ref_rot(rv, 1)) and np.array_equal(bv, ref_rot(ru, 1))
    vu, vv = rot_vector(au, av)      # the vector turn is the face turn with the sign of the new v
    assert np.array_equal(vu, ru) and np.array_equal(vv, -rv)


def test_face_scalar_turn_without_the_reference():
    rng = np.random.default_rng(12)
    au = rng.standard_normal((7, 12)); av = rng.standard_normal((8, 11))
    ru, rv = rot_face(au, av)
    assert np.array_equal(ru, rot(av)) and np.array_equal(rv, rot(au)) and ru.shape == (11, 8) and rv.shape == (12, 7)
    bu, bv = unrot_face(ru, rv)
    assert np.array_equal(bu, au) and np.array_equal(bv, av)


# ---- the oracle and the checkers turn with the grid (CPU) ------------------------------------------------------------------------------------
CPU_CASES = [(o, s) for o, op in OPS.items() for s in op.SETS]


@pytest.mark.parametrize("topo", TOPOS, ids=TOPO_IDS)
@pytest.mark.parametrize("opname,setname", CPU_CASES, ids=[f"{o}-{s}" for o, s in CPU_CASES])
def test_oracle_turns_with_the_grid(opname, setname, topo):
    op = OPS[opname]; opt = op.SETS[setname]
    g, inp = build(op, NI, NJ, topo, {}, opt)
    gr, inp_r = rotate_grid(g), turn(inp, op.VEC, op.FACE)
    assert (gr.ni, gr.nj, gr.reentrant_x, gr.reentrant_y, gr.first_direction) == (g.nj, g.ni, g.reentrant_y, g.reentrant_x, 1 - g.first_direction)
    a = op.oracle(g, inp, opt)
    b = op.oracle(gr, inp_r, opt)
    if not (opname == "hor_visc" and setname in HorVisc.UNCHECKED):
        assert op.worked(g, inp, a), "the operator left its input as it was"
    bad = turning_differences(op, g, a, b)
    assert set(bad) == EXCEPTIONS.get((opname, setname), set()), bad      # (a recorded exception that turns after all comes off the list)


# ---- the library turns with the grid (GPU) ------------------------------------------------------------------------------------------------------
# 70x22 with land, (T,F): six columns past a 64-column tile; its turn is 22x70 and (F,T): narrower than a wave, 70 rows, a topology no parity
# test of these operators has.  26x18, (T,T).  Five tracers where the kernels batch four.
GRIDS = {"70x22_reentrant_x": (70, 22, (True, False)), "26x18_doubly_reentrant": (26, 18, (True, True))}
# Every option set of the operators whose reference is the C oracle (milliseconds each); of the two that are held to the Python checkers
# (seconds each) the sets that reach distinct kernel instantiations: the taper, the EBT structure, both ("neither" is neutral-interior: the
# checker with both switches off is the oracle), HBD with the step and the linear transition and with the EBT structure.
FIVE = dict(ntr=5)
GPU_SIZE = dict(advect=FIVE, hordiff=FIVE, neutral=FIVE, taper_ebt=FIVE)
GPU_SETS = dict({o: list(op.SETS) for o, op in OPS.items()}, taper_ebt=["taper", "ebt", "both"], hbd=["default", "linear", "ebt"])
GPU_CASES = [(o, s, gn, GPU_SIZE.get(o, {})) for o, sets in GPU_SETS.items() for s in sets for gn in GRIDS]
# (the recorded exception names its third tracer: the case of the CPU test)
GPU_CASES = [(o, s, gn, {} if (o, s) == ("neutral", "legacy_20240101") else size) for o, s, gn, size in GPU_CASES]
# many layers: 75 for the neutral surfaces, 31 for the operators that take the layers in chunks of 15
GPU_CASES += [("taper_ebt", "both", "12x8x75", dict(ntr=5, nk=75)), ("hor_visc", "lap_plus_biharm", "26x18x31", dict(nk=31)),
              ("advect", "PPM:H3", "26x18x31", dict(nk=31, ntr=5))]
GRIDS.update({"12x8x75": (12, 8, (True, False)), "26x18x31": (26, 18, (True, True))})


@pytest.mark.gpu
@pytest.mark.parametrize("opname,setname,gridname,size", GPU_CASES, ids=[f"{o}-{s}-{gn}" for o, s, gn, _ in GPU_CASES])
def test_library_turns_with_the_grid(opname, setname, gridname, size):
    """(1) on the turned grid the library is the oracle (the checker), bit for bit; (2) the library's turned-back result on the turned grid is
    its result on the grid, with the same statistics"""
    op = OPS[opname]; opt = op.SETS[setname]
    ni, nj, topo = GRIDS[gridname]
    g, inp = build(op, ni, nj, topo, size, opt)
    gr, inp_r = rotate_grid(g), turn(inp, op.VEC, op.FACE)
    want_r = op.oracle(gr, inp_r, opt)
    dev = Dev()
    try:
        a = op.hip(dev, dev.dg(g), g, inp, opt)
        b = op.hip(dev, dev.dg(gr), gr, inp_r, opt)
    finally:
        dev.close()
    if not (opname == "hor_visc" and setname in HorVisc.UNCHECKED):
        assert op.worked(g, inp, a), "the operator left its input as it was"
    bad = differences(gr, want_r, b, bits_equal)
    assert not bad, ("the library is not the oracle on the turned grid", bad)
    bad = set(turning_differences(op, g, a, b)) - GPU_EXCEPTIONS.get((opname, setname), set())
    assert not bad, ("the library does not turn with the grid", sorted(bad))
