"""continuity_PPM: CPU checks of the oracle (oracle/continuity.c) through what the scheme guarantees, and GPU
parity of libmom6hip against the oracle (bit-exact fp64).  The reference holds no known-answer vectors for
continuity_PPM (parity unpinned)."""
import numpy as np
import pytest

from mom6_amd import _abi, synth
from helpers import bits_equal, interior


def cont_case(ni=40, nj=28, nk=4, seed=2, first_direction=0, **kw):
    g = synth.make_grid(ni, nj, nk, seed=seed + 10, first_direction=first_direction, **kw)
    st = {k: v.numpy() for k, v in synth.make_dynamics_state(g, seed=seed).items()}
    rng = np.random.default_rng(seed)
    kk = (np.arange(nk) + 0.5) / nk
    vr = np.clip(1.0 - 0.8 * kk[:, None, None] ** 4 + 0.0 * st["u"], 0.05, 1.0)
    st["visc_rem_u"] = np.ascontiguousarray(vr * (0.9 + 0.1 * rng.random(st["u"].shape)))
    vr = np.clip(1.0 - 0.8 * kk[:, None, None] ** 4 + 0.0 * st["v"], 0.05, 1.0)
    st["visc_rem_v"] = np.ascontiguousarray(vr * (0.9 + 0.1 * rng.random(st["v"].shape)))
    return g, st


def run_oracle(orc, g, st, dt=900.0, with_bt=True, with_uhbt=True, with_visc=True, with_h=True, alias=False, **cskw):
    cs = orc.continuity_cs(g.nk, g.Angstrom_H, **cskw)
    h = st["h"].copy()
    hin = h if alias else st["h"].copy()
    uh, vh = np.zeros_like(st["u"]), np.zeros_like(st["v"])
    out = {"h": h, "uh": uh, "vh": vh}
    kw = {}
    if with_visc:
        kw.update(visc_rem_u=st["visc_rem_u"], visc_rem_v=st["visc_rem_v"])
    if with_uhbt:
        # a first call without uhbt gives the layer-summed transports; perturb them to make the solver work
        orc.continuity(g, cs, st["u"], st["v"], st["h"].copy(), st["h"].copy(), uh, vh, dt, **kw)
        out["uhbt"] = np.ascontiguousarray(uh.sum(0) * 1.05 + 0.02 * np.abs(uh).sum(0))
        out["vhbt"] = np.ascontiguousarray(vh.sum(0) * 0.95 - 0.02 * np.abs(vh).sum(0))
        uh[:] = 0; vh[:] = 0
        out.update(u_cor=np.zeros_like(st["u"]), v_cor=np.zeros_like(st["v"]), du_cor=g.zeros2(_abi.POS_U),
                   dv_cor=g.zeros2(_abi.POS_V))
        kw.update(uhbt=out["uhbt"], vhbt=out["vhbt"], u_cor=out["u_cor"], v_cor=out["v_cor"], du_cor=out["du_cor"],
                  dv_cor=out["dv_cor"])
    if with_bt:
        arrs, btst = orc.make_bt_cont(g, with_h=with_h)
        out["bt"] = arrs
        kw["bt_cont"] = btst
    orc.continuity(g, cs, st["u"], st["v"], hin, h, uh, vh, dt, **kw)
    return out


def test_mass_conservation_and_positivity(oracle):
    g, st = cont_case()
    out = run_oracle(oracle, g, st, with_bt=False, with_uhbt=False)
    A = g.areaT
    m0 = interior(g, st["h"] * A).sum(); m1 = interior(g, out["h"] * A).sum()
    assert abs(m1 - m0) < 1e-12 * m0
    assert interior(g, out["h"]).min() >= g.Angstrom_H


def test_barotropic_transport_is_matched(oracle):
    g, st = cont_case()
    out = run_oracle(oracle, g, st, with_bt=False)
    dt = 900.0
    errx = interior(g, (out["uh"].sum(0) - out["uhbt"]), _abi.POS_U)
    IA = interior(g, g.IareaT).max()
    tol = 0.5 * g.nk * g.Angstrom_H
    # flux_adjust stops when dt*min(IareaT)*|err| <= tol_eta (:1187)
    assert np.max(np.abs(errx)) * dt * IA <= 4 * tol
    erry = interior(g, (out["vh"].sum(0) - out["vhbt"]), _abi.POS_V)
    assert np.max(np.abs(erry)) * dt * IA <= 4 * tol
    # u_cor = u + du*visc_rem (:744)
    k = 1
    lhs = interior(g, out["u_cor"][k], _abi.POS_U)
    rhs = interior(g, st["u"][k] + out["du_cor"] * st["visc_rem_u"][k], _abi.POS_U)
    assert bits_equal(lhs, rhs)


def test_bt_cont_is_sane(oracle):
    g, st = cont_case()
    out = run_oracle(oracle, g, st)
    bt = out["bt"]
    for n in ("FA_u_W0", "FA_u_WW", "FA_u_E0", "FA_u_EE"):
        a = interior(g, bt[n], _abi.POS_U)
        assert np.all(a >= 0.0) and np.all(np.isfinite(a)) and a.max() > 0
    assert np.all(interior(g, bt["uBT_WW"], _abi.POS_U) >= 0.0) and np.all(interior(g, bt["uBT_EE"], _abi.POS_U) <= 0.0)
    assert interior(g, bt["h_u"], _abi.POS_U).max() > 0


def test_visc_rem_must_come_in_pairs(oracle):
    g, st = cont_case(ni=12, nj=10, nk=2)
    cs = oracle.continuity_cs(g.nk)
    with pytest.raises(RuntimeError, match="Either both visc_rem_u and visc_rem_v"):
        oracle.continuity(g, cs, st["u"], st["v"], st["h"], st["h"].copy(), np.zeros_like(st["u"]),
                          np.zeros_like(st["v"]), 900.0, visc_rem_u=st["visc_rem_u"])


VARIANTS = [
    dict(),                                            # defaults: PPM + positive-definite limiter
    dict(monotonic=1),
    dict(simple_2nd=1),
    dict(upwind_1st=1),
    dict(aggress_adjust=1),
    dict(vol_CFL=1, better_iter=0, use_visc_rem_max=0, marginal_faces=0),
]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", range(len(VARIANTS)))
@pytest.mark.parametrize("first_direction", [0, 1])
def test_gpu_parity(oracle, variant, first_direction):
    import torch
    from mom6_amd.continuity import BT_cont_type, continuity
    from mom6_amd.tracer_advect import DeviceGrid
    cskw = VARIANTS[variant]
    # nk = 20 and 75 reach the 4-layers-per-slab form and the deep forms (zonally 8 waves x 5 layers, meridionally 4 waves x 10 layers)
    # of the block-cooperative flux kernels, with the last slabs partly filled; nk = 83 and 90 are past their 80 layers and take the
    # lane-per-column kernels
    # the last grid has halo = the PPM stencil (3): the first pass then runs to the very edge of the data domain
    for (ni, nj, nk, topo, halo) in [(70, 21, 4, (True, False), 4), (44, 40, 2, (True, True), 4), (10, 8, 8, (False, False), 4),
                                     (36, 13, 20, (True, True), 4), (67, 9, 75, (True, False), 4), (14, 9, 90, (True, False), 4),
                                     (61, 12, 12, (True, True), 3), (33, 8, 83, (True, False), 4)]:
        g, st = cont_case(ni, nj, nk, seed=ni, first_direction=first_direction, reentrant_x=topo[0], reentrant_y=topo[1], halo=halo)
        dg = DeviceGrid(g)
        cs = oracle.continuity_cs(g.nk, g.Angstrom_H, **cskw)
        for mode in ("plain", "uhbt", "bt_cont", "all", "all_novisc", "alias"):
            kw = dict(with_bt=mode in ("bt_cont", "all", "all_novisc"), with_uhbt=mode in ("uhbt", "all", "all_novisc", "alias"),
                      with_visc=mode != "all_novisc", alias=mode == "alias")
            ref = run_oracle(oracle, g, st, **kw, **cskw)
            for resident in (False, True):
                X = (lambda a: None if a is None else torch.from_numpy(a.copy()).cuda()) if resident else \
                    (lambda a: None if a is None else a.copy())
                h = X(st["h"]); hin = h if kw["alias"] else X(st["h"])
                uh, vh = X(np.zeros_like(st["u"])), X(np.zeros_like(st["v"]))
                args = {}
                if kw["with_visc"]:
                    args.update(visc_rem_u=X(st["visc_rem_u"]), visc_rem_v=X(st["visc_rem_v"]))
                if kw["with_uhbt"]:
                    args.update(uhbt=X(ref["uhbt"]), vhbt=X(ref["vhbt"]), u_cor=X(np.zeros_like(st["u"])),
                                v_cor=X(np.zeros_like(st["v"])), du_cor=X(g.zeros2(_abi.POS_U)), dv_cor=X(g.zeros2(_abi.POS_V)))
                bt = None
                if kw["with_bt"]:
                    arrs, _ = oracle.make_bt_cont(g, with_h=True)
                    bt = BT_cont_type(**{n: X(a) for n, a in arrs.items()})
                    args["BT_cont"] = bt
                continuity(X(st["u"]), X(st["v"]), hin, h, uh, vh, 900.0, dg, cs, **args)
                dg.sync()
                N = (lambda a: a.cpu().numpy()) if resident else (lambda a: a)
                what = (variant, first_direction, (ni, nj, nk), mode, resident)
                for name, arr in (("h", h), ("uh", uh), ("vh", vh)):
                    assert bits_equal(ref[name], N(arr)), (what, name, np.argwhere(ref[name] != N(arr))[:3])
                if kw["with_uhbt"]:
                    for name in ("u_cor", "v_cor", "du_cor", "dv_cor"):
                        assert bits_equal(ref[name], N(args[name])), (what, name, np.argwhere(ref[name] != N(args[name]))[:3])
                if bt is not None:
                    for name, arr in bt.arrays.items():
                        assert bits_equal(ref["bt"][name], N(arr)), (what, name, np.argwhere(ref["bt"][name] != N(arr))[:3])
        dg.close()
