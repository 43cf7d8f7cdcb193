"""pgf_face_kernel_t, the face kernel of PressureForce_FV_Bouss with its options fixed at compile time (EQN_OF_STATE = WRIGHT x
MASS_WEIGHT_IN_PRESSURE_GRADIENT x a surface pressure x the RK2 step's u_bc_accel fused in: off / viscous / inviscid): the library
equals the oracle bit for bit in every instantiation, the instantiation (and not the generic pgf_face_kernel) is what was
launched (mom6hip_pgf_face_launches), and a form without an instantiation still takes the generic kernel."""
import numpy as np
import pytest

from mom6_amd import _abi, synth
from helpers import bits_equal

# (ni, nj, nk, reentrant_x, reentrant_y): nk = 2 (the layer loop's first layer, then its last), 5, 75 (the benchmark's depth); widths
# that are not a multiple of 64 (one partial wave; a full wave followed by a partial one).  nk = 1 cannot reach this kernel: see
# test_one_layer_is_refused.
SHAPES = [(70, 21, 5, True, False), (44, 12, 2, True, True), (130, 9, 75, True, False), (37, 8, 2, False, False)]


def _case(ni, nj, nk, rx, ry):
    g = synth.make_grid(ni, nj, nk, seed=ni + 10, reentrant_x=rx, reentrant_y=ry)      # land_frac 0.2 by default
    st = {k: v.numpy() for k, v in synth.make_dynamics_state(g, seed=ni).items()}      # 5 % vanished layers (h = Angstrom_H)
    return g, st


def _hwght_x(g, h):
    """hWght of the x faces (MOM_density_integrals.F90:606) before its scaling, [k, j, I] over the h points but the last column"""
    e = np.empty((g.nk + 1,) + h.shape[1:]); e[g.nk] = -g.bathyT
    for k in range(g.nk - 1, -1, -1):
        e[k] = e[k + 1] + h[k] * g.H_to_Z
    bL, bR = g.bathyT[:, :-1], g.bathyT[:, 1:]
    return np.maximum(0.0, np.maximum(-bL[None] - e[:-1, :, 1:], -bR[None] - e[:-1, :, :-1]))


def test_cases_hold_what_the_kernel_must_handle():
    """the inputs of the GPU tests below: land, vanished layers, and rows where one wave (64 consecutive x faces) holds faces with
    hWght > 0 beside faces with hWght = 0"""
    ni, nj, nk, rx, ry = SHAPES[0]
    g, st = _case(ni, nj, nk, rx, ry)
    sj, si = g.csl(_abi.POS_H)
    assert (g.mask2dT[sj, si] == 0).any() and (g.mask2dT[sj, si] > 0).any()
    assert (st["h"][:, sj, si] == g.Angstrom_H).any()
    hw = _hwght_x(g, st["h"])[:, sj, si.start - 1:si.start + 63]      # the first wave of every interior row
    assert ((hw > 0).any(axis=2) & (hw == 0).any(axis=2)).any(), "no wave with hWght > 0 and hWght = 0 side by side"


@pytest.mark.gpu
@pytest.mark.parametrize("p_atm_on", [False, True], ids=["no_p_atm", "p_atm"])
@pytest.mark.parametrize("massw", [False, True], ids=["plain", "massw"])
@pytest.mark.parametrize("form", ["WRIGHT", "UNESCO"])
def test_pressureforce_specialised_equals_oracle(oracle, form, massw, p_atm_on):
    """PressureForce_FV_Bouss alone (no u_bc_accel): WRIGHT runs pgf_face_kernel_t<WRIGHT, massw, off, p_atm>, UNESCO the generic kernel"""
    import torch
    from mom6_amd.pressure_force import PressureForce, PressureForce_init, EOS_init, pgf_face_launches
    from mom6_amd.tracer_advect import DeviceGrid
    for (ni, nj, nk, rx, ry) in SHAPES:
        g, st = _case(ni, nj, nk, rx, ry)
        E = oracle.eos(form, 1000.0, -0.2, 0.8)
        cs = oracle.pressureforce_cs(g, boundary_extrap=True, useMassWghtInterp=massw)
        rng = np.random.default_rng(ni)
        p_atm = np.ascontiguousarray(1.0e5 + 500.0 * rng.standard_normal(g.shape2(_abi.POS_H))) if p_atm_on else None
        ref = oracle.pressureforce(g, cs, E, st["h"], st["T"], st["S"], p_atm)
        dg = DeviceGrid(g)
        CS = PressureForce_init(g, boundary_extrap=True, useMassWghtInterp=massw)
        EOS = EOS_init(form, 1000.0, -0.2, 0.8)
        for resident in (False, True):
            X = (lambda a: None if a is None else torch.from_numpy(a.copy()).cuda()) if resident else \
                (lambda a: None if a is None else a.copy())
            PFu, PFv = X(g.zeros3(_abi.POS_U)), X(g.zeros3(_abi.POS_V))
            pbce, eta = X(g.zeros3(_abi.POS_H)), X(g.zeros2(_abi.POS_H))
            before = pgf_face_launches(dg)
            PressureForce(X(st["h"]), (X(st["T"]), X(st["S"]), EOS), PFu, PFv, dg, CS, p_atm=X(p_atm), pbce=pbce, eta=eta)
            dg.sync()
            after = pgf_face_launches(dg)
            want = (0, 1) if form == "WRIGHT" else (1, 0)
            assert (after[0] - before[0], after[1] - before[1]) == want, (form, (ni, nj, nk), resident, before, after)
            N = (lambda a: a.cpu().numpy()) if resident else (lambda a: a)
            for name, a, b in (("PFu", ref[0], PFu), ("PFv", ref[1], PFv), ("pbce", ref[2], pbce), ("eta", ref[3], eta)):
                assert bits_equal(a, N(b)), (form, massw, (ni, nj, nk), p_atm_on, resident, name, np.argwhere(a != N(b))[:3])
        dg.close()


@pytest.mark.gpu
def test_one_layer_is_refused():
    """nk = 1 is outside PressureForce_FV_Bouss with the PLM reconstruction: the entry point requires 2 layers and refuses before any
    kernel is launched, so the face kernels' layer loop starts at nk = 2"""
    import torch
    from mom6_amd._lib import Mom6HipError
    from mom6_amd.pressure_force import PressureForce, PressureForce_init, EOS_init, pgf_face_launches
    from mom6_amd.tracer_advect import DeviceGrid
    g, st = _case(37, 8, 1, False, False)
    dg = DeviceGrid(g)
    X = lambda a: torch.from_numpy(a.copy()).cuda()
    with pytest.raises(Mom6HipError, match="at least 2 layers"):
        PressureForce(X(st["h"]), (X(st["T"]), X(st["S"]), EOS_init("WRIGHT")), X(g.zeros3(_abi.POS_U)), X(g.zeros3(_abi.POS_V)), dg,
                      PressureForce_init(g))
    assert pgf_face_launches(dg) == (0, 0)
    dg.close()


def _rk2_steps_equal_oracle(orc, shapes, viscous, form, pf, p_surf_on, want):
    """three steps of step_MOM_dyn_split_RK2 with EQN_OF_STATE = form and the PressureForce options pf (the oracle's names) on each
    shape: u, v, h, uh, eta_av are the oracle's bit for bit, and the face kernel launch counter moved by want = (run-time PLM
    kernel, pgf_face_kernel_t)"""
    import torch
    from mom6_amd.dynamics_split_rk2 import initialize_dyn_split_RK2, step_MOM_dyn_split_RK2
    from mom6_amd.pressure_force import pgf_face_launches
    from mom6_amd.tracer_advect import DeviceGrid
    from mom6_amd.vert_friction import vertvisc_type
    for (ni, nj, nk) in shapes:
        g = synth.make_grid(ni, nj, nk, seed=ni + 1)
        d = {k: v.numpy() for k, v in synth.make_dynamics_state(g, seed=3, umax=0.1, eta_amp=0.2).items()}
        taux = np.ascontiguousarray(0.1 * g.mask2dCu); tauy = g.zeros2(_abi.POS_V)
        dt = 1800.0
        rng = np.random.default_rng(5)
        su, sv = g.shape2(_abi.POS_U), g.shape2(_abi.POS_V)
        va = dict(Kv_bbl_u=1.0e-3 * (0.5 + rng.random(su)), Kv_bbl_v=1.0e-3 * (0.5 + rng.random(sv)),
                  bbl_thick_u=2.0 + 8.0 * rng.random(su), bbl_thick_v=2.0 + 8.0 * rng.random(sv))
        okw, lkw = {}, {}
        if viscous:
            okw = dict(vertvisc=orc.vertvisc_cs(g, Kv=1.0e-3, Hbbl=10.0), visc=orc.vertvisc_type(**va),
                       hor_visc=orc.hor_visc_cs(g, dt, biharmonic=1, Smagorinsky_Ah=1, Smag_bi_const=0.06, Ah_vel_scale=0.01))
            lkw = dict(vertvisc=dict(KV=1.0e-3, HBBL=10.0),
                       hor_visc=dict(BIHARMONIC=True, SMAGORINSKY_AH=True, SMAG_BI_CONST=0.06, AH_VEL_SCALE=0.01))
        ref = orc.DynState(g, d["u"], d["v"], d["h"], d["T"], d["S"], dt, eos_form=form, pressureforce=dict(pf), **okw)
        p_surf = None
        if p_surf_on:
            p_surf = np.ascontiguousarray(1.0e5 + 200.0 * rng.standard_normal(g.shape2(_abi.POS_H)))
            orc.halo_update(g, p_surf, _abi.POS_H)
        dg = DeviceGrid(g)
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        u, v, h, Tt, Ss = (T(d[k]) for k in ("u", "v", "h", "T", "S"))
        Z = lambda pos, k3=True: torch.zeros(g.shape3(pos) if k3 else g.shape2(pos), dtype=torch.float64, device="cuda")
        uh, vh, uhtr, vhtr, eta_av = Z(_abi.POS_U), Z(_abi.POS_V), Z(_abi.POS_U), Z(_abi.POS_V), Z(_abi.POS_H, False)
        CS = initialize_dyn_split_RK2(u, v, h, uh, vh, dt, dg, coriolis=dict(bound_coriolis=True), EQN_OF_STATE=form,
                                      pressure_force=dict(pf), **lkw)
        visc = vertvisc_type(**{n: T(a) for n, a in va.items()}) if viscous else None
        tx, ty = T(taux), T(tauy)
        before = pgf_face_launches(dg)
        nstep = 3
        for n in range(nstep):
            ref.step(taux, tauy, calc_dtbt=(n == 0), p_surf=p_surf)
            forces = (tx, ty) if p_surf is None else (tx, ty, T(p_surf))
            step_MOM_dyn_split_RK2(u, v, h, (Tt, Ss), visc, None, dt, forces, None, None, uh, vh, uhtr, vhtr, eta_av, dg, CS,
                                   calc_dtbt=(n == 0))
        dg.sync()
        after = pgf_face_launches(dg)
        assert (after[0] - before[0], after[1] - before[1]) == (want[0] * nstep, want[1] * nstep), (before, after)
        for name, a, b in (("u", u, ref.u), ("v", v, ref.v), ("h", h, ref.h), ("uh", uh, ref.uh), ("eta_av", eta_av, ref.eta_av)):
            assert bits_equal(a.cpu().numpy(), b), (form, pf, viscous, p_surf_on, (ni, nj, nk), name)
        dg.close()


@pytest.mark.gpu
@pytest.mark.parametrize("p_surf_on", [False, True], ids=["no_p_surf", "p_surf"])
@pytest.mark.parametrize("massw", [False, True], ids=["plain", "massw"])
@pytest.mark.parametrize("viscous", [True, False], ids=["viscous", "inviscid"])
def test_rk2_step_with_bc_accel_fused_equals_oracle(oracle, viscous, massw, p_surf_on):
    """step_MOM_dyn_split_RK2 from its second step on hands u_bc_accel = (CAu_pred + PFu) + diffu to the face kernel: with
    horizontal and vertical viscosity pgf_face_kernel_t<WRIGHT, massw, viscous, p_surf>, without either <.., inviscid, ..>"""
    _rk2_steps_equal_oracle(oracle, [(70, 12, 2), (30, 10, 75)], viscous, "WRIGHT", dict(useMassWghtInterp=massw), p_surf_on, (0, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("viscous", [True, False], ids=["viscous", "inviscid"])
def test_rk2_step_with_bc_accel_fused_in_the_run_time_kernel_equals_oracle(oracle, viscous):
    """EQN_OF_STATE = UNESCO has no pgf_face_kernel_t: the run-time face kernel with the PLM quadrature forms u_bc_accel, in its
    viscous and its inviscid form (nk = 2: the layer loop's first layer, then its last; 70: a full wave and a partial one)"""
    _rk2_steps_equal_oracle(oracle, [(70, 12, 2), (30, 10, 5)], viscous, "UNESCO", {}, False, (1, 0))


@pytest.mark.gpu
def test_rk2_step_without_reconstruction_equals_oracle(oracle):
    """RECONSTRUCT_FOR_PRESSURE = False with EQN_OF_STATE = LINEAR: the run-time face kernel with the analytic integral of the linear
    form, which is not handed u_bc_accel (the step forms it) and is not counted as a PLM launch"""
    _rk2_steps_equal_oracle(oracle, [(70, 12, 2)], True, "LINEAR", dict(reconstruct=False), False, (0, 0))
