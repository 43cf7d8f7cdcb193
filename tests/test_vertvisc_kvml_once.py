"""The KV_ML_INVZ2 viscosity profile formed once a step: the first of the step's three vertical-viscosity calls forms it, the other two
read it (mom6_amd/csrc/dyn_split_rk2.hip, m6::KvmlProfile).  The thicknesses change from step to step, so a profile carried across
a step would show against the oracle, which forms the profile in every call; MOM6HIP_VV_KVML_ONCE=0 is the library doing the same.

The switch is read once a process: every GPU run here is a fresh child process (this file run as a script), which steps the model
and leaves the fields of every step in an .npz; the test compares them bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NSTEP = 4
FIELDS = ("u", "v", "h", "uh", "vh", "eta_av", "visc_rem_u", "visc_rem_v", "a_u", "a_v")
VV = dict(KV=1.0e-3, HBBL=10.0, HMIX_FIXED=20.0, KV_ML_INVZ2=1.0e-2)
DT = 1800.0
REPORT = "KV_ML_INVZ2 profile arrays reserved"

CASES = {
    # a viscous RK2 step with KV_ML_INVZ2 > 0 and HMIX_FIXED > 0
    "rk2": dict(grid=dict(ni=26, nj=18, nk=6, seed=6), rk2b=False, vv=VV),
    # the same with SPLIT_RK2B
    "rk2b": dict(grid=dict(ni=44, nj=40, nk=2, seed=4, reentrant_y=True), rk2b=True, vv=VV),
    # mostly land on the benchmark's re-entrant grid: masked columns run no coefficient sweep in any of the three calls
    "land": dict(grid=dict(ni=40, nj=24, nk=5, seed=11, reentrant_x=True, land_frac=0.6), rk2b=False, vv=VV),
    # no KV_ML_INVZ2: nothing to keep, and nothing reserved for it (no wind: nothing would spread its stress below a thin top layer)
    "no_kvml": dict(grid=dict(ni=26, nj=18, nk=6, seed=6), rk2b=False, vv=dict(VV, KV_ML_INVZ2=0.0), wind=0.0),
}


def _case(cfg):
    from mom6_amd import _abi, synth
    kw = dict(ni=20, nj=16, nk=3, seed=4, reentrant_x=True, reentrant_y=False, land_frac=0.2)
    kw.update(cfg["grid"])
    seed = kw.pop("seed")
    g = synth.make_grid(kw.pop("ni"), kw.pop("nj"), kw.pop("nk"), seed=seed + 300, **kw)
    d = {k: v.numpy() for k, v in synth.make_dynamics_state(g, seed=seed, umax=0.1, eta_amp=0.2).items()}
    yy = np.linspace(0.0, np.pi, g.shape2(_abi.POS_U)[0])
    taux = np.ascontiguousarray(cfg.get("wind", 0.1) * np.cos(2 * yy)[:, None] * g.mask2dCu)
    tauy = np.ascontiguousarray(0.0 * g.mask2dCv)
    rng = np.random.default_rng(9)
    su, sv = g.shape2(_abi.POS_U), g.shape2(_abi.POS_V)
    va = dict(Kv_bbl_u=1.0e-3 * (0.5 + rng.random(su)), Kv_bbl_v=1.0e-3 * (0.5 + rng.random(sv)),
              bbl_thick_u=2.0 + 8.0 * rng.random(su), bbl_thick_v=2.0 + 8.0 * rng.random(sv))
    return g, d, taux, tauy, va


def _oracle_steps(cfg):
    from oracle import orc
    g, d, taux, tauy, va = _case(cfg)
    vv = cfg["vv"]
    ref = orc.DynState(g, d["u"], d["v"], d["h"], d["T"], d["S"], DT, rk2b=cfg["rk2b"],
                       vertvisc=orc.vertvisc_cs(g, Kv=vv["KV"], Hbbl=vv["HBBL"], Hmix=vv["HMIX_FIXED"], Kvml_invZ2=vv["KV_ML_INVZ2"]),
                       visc=orc.vertvisc_type(**va))
    ref.bcs.dtbt = DT / 9.6
    out = {}
    for n in range(NSTEP):
        ref.step(taux, tauy)
        now = dict(u=ref.u, v=ref.v, h=ref.h, uh=ref.uh, vh=ref.vh, eta_av=ref.eta_av, visc_rem_u=ref.arrs["visc_rem_u"],
                   visc_rem_v=ref.arrs["visc_rem_v"], a_u=ref.vvcs._arrs["a_u"], a_v=ref.vvcs._arrs["a_v"])
        out.update({f"{k}{n}": np.array(a, copy=True) for k, a in now.items()})
    return g, out


def _gpu_steps(cfg, path):
    """(child process) NSTEP steps on the GPU; the fields after every step go to `path`"""
    import torch
    from mom6_amd import _abi
    from mom6_amd.dynamics_split_rk2 import (initialize_dyn_split_RK2, initialize_dyn_split_RK2b, step_MOM_dyn_split_RK2,
                                             step_MOM_dyn_split_RK2b)
    from mom6_amd.tracer_advect import DeviceGrid
    from mom6_amd.vert_friction import vertvisc_type
    g, d, taux, tauy, va = _case(cfg)
    rk2b = cfg["rk2b"]
    dg = DeviceGrid(g)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    u, v, h, Tt, Ss = (T(d[k]) for k in ("u", "v", "h", "T", "S"))
    Z = lambda pos, k3=True: torch.zeros(g.shape3(pos) if k3 else g.shape2(pos), dtype=torch.float64, device="cuda")
    uh, vh, uhtr, vhtr, eta_av = Z(_abi.POS_U), Z(_abi.POS_V), Z(_abi.POS_U), Z(_abi.POS_V), Z(_abi.POS_H, False)
    CS = (initialize_dyn_split_RK2b if rk2b else initialize_dyn_split_RK2)(u, v, h, uh, vh, DT, dg, coriolis=dict(bound_coriolis=True),
                                                                           vertvisc=dict(cfg["vv"]))
    CS.barotropic_CSp.st.dtbt = DT / 9.6
    visc = vertvisc_type(**{n: T(a) for n, a in va.items()})
    tx, ty = T(taux), T(tauy)
    step = step_MOM_dyn_split_RK2b if rk2b else step_MOM_dyn_split_RK2
    out = {}
    for n in range(NSTEP):
        step(u, v, h, (Tt, Ss), visc, None, DT, (tx, ty), None, None, uh, vh, uhtr, vhtr, eta_av, dg, CS)
        dg.sync()
        now = dict(u=u, v=v, h=h, uh=uh, vh=vh, eta_av=eta_av, visc_rem_u=CS.visc_rem_u, visc_rem_v=CS.visc_rem_v,
                   a_u=CS.vertvisc_CSp.a_u, a_v=CS.vertvisc_CSp.a_v)
        out.update({f"{k}{n}": a.cpu().numpy().copy() for k, a in now.items()})
    dg.close()
    np.savez(path, **out)


def _child(name, path, once):
    """Runs case `name` in a fresh process with MOM6HIP_VV_KVML_ONCE unset (once) or 0; returns what it wrote and its stderr"""
    env = dict(os.environ)
    env.pop("MOM6HIP_VV_KVML_ONCE", None)
    if not once:
        env["MOM6HIP_VV_KVML_ONCE"] = "0"
    env["MOM6HIP_VV_KVML_REPORT"] = "1"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), name, str(path)]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (name, once, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    with np.load(str(path)) as z:
        return {k: z[k] for k in z.files}, r.stderr


def _same(a, b, what):
    from helpers import bits_equal
    for n in range(NSTEP):
        for k in FIELDS:
            x, y = a[f"{k}{n}"], b[f"{k}{n}"]
            assert x.shape == y.shape and bits_equal(x, y), (what, "step", n, k, float(np.abs(x - y).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rk2", "rk2b", "land"])
def test_profile_formed_once_a_step_matches_oracle_and_every_call_forming_it(name, tmp_path):
    cfg = CASES[name]
    g, ref = _oracle_steps(cfg)
    once, err_once = _child(name, tmp_path / "once.npz", True)
    each, err_each = _child(name, tmp_path / "each.npz", False)
    for n in range(1, NSTEP):      # the thicknesses do change between the steps: a profile kept across one would be another profile
        assert not np.array_equal(ref[f"h{n}"], ref[f"h{n - 1}"])
    if name == "land":
        from mom6_amd import _abi
        from helpers import interior
        wet = float((interior(g, np.asarray(g.mask2dCu), _abi.POS_U) > 0).mean())
        assert 0.0 < wet < 0.5, wet
    _same(once, ref, "formed once a step against the oracle")
    _same(each, ref, "formed by every call against the oracle")
    _same(once, each, "formed once a step against formed by every call")
    # the two arrays are reserved by the stepper that hands the profile on, and only by it
    assert err_once.count(REPORT) == 1, err_once[-2000:]
    assert REPORT not in err_each, err_each[-2000:]


@pytest.mark.gpu
def test_without_kv_ml_invz2_nothing_is_reserved(tmp_path):
    g, ref = _oracle_steps(CASES["no_kvml"])
    once, err = _child("no_kvml", tmp_path / "once.npz", True)
    _same(once, ref, "KV_ML_INVZ2 = 0 against the oracle")
    assert REPORT not in err, err[-2000:]


if __name__ == "__main__":
    for p in (ROOT, HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    _gpu_steps(CASES[sys.argv[1]], sys.argv[2])
