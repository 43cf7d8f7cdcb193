"""The thickness unit (tests/rescaling.py: the reference's H_RESCALE_POWER / .testing `test.dim.h` property) under every operator and
under the step.  Each operator runs on a grid g and on rescale_grid(g, c), where a thickness is a number 2^c times as large, with every
input times 2^(c e), e the power of H in the input's units; every entry of the result has to be the unit result times 2^(c e) of its own
units, to the bit on the compute domain, with the same counts (iterations, truncations, nstep) and the same dtbt.  Options given in
metres or m2 s-1 (HBBL, HMIX_FIXED, KV, KHTH, ...) are the same in both runs: the set-up functions convert them with GV%Z_to_H.

c = 11 is the power of the reference's own test.dim.h; c = -7 runs with each operator's first option set.

On the CPU (no mark) the property is established for the oracle and the Python checkers.  On the GPU the library is held to (1) parity
with the oracle / checker on the SCALED grid, bit for bit -- the only place where the kernels meet H_to_Z != 1 beside the oracle -- and
(2) the scaling of its own results.

The table DIMS of each operator gives the power of H of every input, output and scalar result, with the declaration in the reference that
states the units.  No option set is recorded as an exception: every entry of every one scales.
"""
import functools

import numpy as np
import pytest

import test_barotropic as tbt
import test_properties as tp
import test_regridding as treg
import test_sum_output as tso
import test_rotation_tracers_params as trp
from helpers import barotropic_case, bits_equal, interior
from mom6_amd import _abi
from oracle import orc
from rescaling import rescale_grid, scale_fields
from test_rotation_tracers_params import Dev, differences, dom

H, U, V = _abi.POS_H, _abi.POS_U, _abi.POS_V
NI, NJ, TOPO = 26, 18, (True, False)
GPU_NI, GPU_NJ = 70, 22
POWERS = (11, -7)

# ---- the power of H in the units of every named field, operator by operator (reference: /src) ------------------------------------------------
# Shared declarations: h [H ~> m or kg m-2]; uhtr, vhtr [H L2 ~> m3 or kg]; u, v [L T-1]; T, S, tr: concentrations; the VarMix fields of
# parameterizations/lateral/MOM_lateral_mixing_coeffs.F90:78-115 (SN_u [T-1], L2u [L2], cg1 [L T-1], Rd_dx_h, Res_fn, Depth_fn, ebt_struct
# [nondim], slope_x [Z L-1]) and the MEKE fields of MOM_MEKE_types.F90:11-23 (GM_src, mom_src [R Z L2 T-3], Kh, Ku [L2 T-1], Au [L4 T-1]) hold
# no thickness.
VARMIX = dict(L2u=0, L2v=0, SN_u=0, SN_v=0, Res_fn_h=0, Rd_dx_h=0, Kh=0, Res_fn_u=0, Res_fn_v=0, slope_x=0, slope_y=0, cg1=0, Depth_fn_u=0, Depth_fn_v=0,
              MEKE_Kh=0, ebt=0)
DIMS = dict(
    # tracer/MOM_tracer_advect.F90:57 h_end [H], :59-64 uhtr, vhtr [H L2], :73 vol_prev [H L2], :82-87 uhr_out, vhr_out [H L2]
    advect=dict(h_end=1, uhtr=1, vhtr=1, vol0=1, tr=0, vol=1, uhr=1, vhr=1, stats=0),
    # tracer/MOM_tracer_hor_diff.F90:123 h [H]; KhTr and its kin are [L2 T-1]
    hordiff=dict(VARMIX, h=1, tr=0, stats=0),
    # tracer/MOM_neutral_diffusion.F90:341 h [H], :64 hbl [H] (= visc%h_ML, core/MOM_variables.F90:268 [H]), :343 p_surf [R L2 T-2]
    neutral=dict(h=1, tr=0, h_ML=1, p_surf=0, stats=0),
    taper_ebt=dict(VARMIX, h=1, tr=0, h_ML=1, stats=0),
    # tracer/MOM_hor_bnd_diffusion.F90:181 hbl [H] (= visc%h_ML)
    hbd=dict(VARMIX, h=1, tr=0, h_ML=1, stats=0),
    # tracer/MOM_tracer_hor_diff.F90:704 h [H]; GV%Rlay [R]
    epipycnal=dict(h=1, tr=0, eos=None, Rlay=0, stats=0),
    # parameterizations/lateral/MOM_thickness_diffuse.F90:137 h [H], :138-141 uhtr, vhtr [H L2], :646-649 uhD, vhD [H L2 T-1] (= CDp%uhGM)
    thickness_diffuse=dict(VARMIX, h=1, u=0, v=0, T=0, S=0, tr=0, uhtr=1, vhtr=1, uhGM=1, vhGM=1, GM_src=0),
    # parameterizations/lateral/MOM_mixed_layer_restrat.F90:139 h [H], :140-143 uhtr, vhtr [H L2], :149-151 h_MLD [H], :103-104 MLD_filtered,
    # MLD_filtered_slow [H], :195 uhml [H L2 T-1]; forces%ustar [Z T-1], core/MOM_forcing_type.F90:265 (find_ustar turns it into [H T-1], :286)
    restrat=dict(h=1, u=0, v=0, T=0, S=0, tr=0, ustar=0, h_MLD=1, Rd_dx_h=0, MLD_filtered=1, MLD_filtered_slow=1, uhtr=1, vhtr=1, uhml=1, vhml=1),
    # parameterizations/lateral/MOM_hor_visc.F90:254 h [H], :256 diffu [L T-2], :274 hu_cont [H]
    hor_visc=dict(h=1, u=0, v=0, T=0, S=0, tr=0, hu_cont=1, hv_cont=1, Ku=0, Au=0, mom_src=0, diffu=0, diffv=0),
    # core/MOM_variables.F90:235-236 bbl_thick_u [Z], :237-238 kv_bbl_u [H Z T-1], :263-264 Ray_u [H T-1]
    set_viscous_BBL=dict(h=1, u=0, v=0, T=0, S=0, tr=0, Kv_bbl_u=1, Kv_bbl_v=1, bbl_thick_u=0, bbl_thick_v=0, Ray_u=1, Ray_v=1),
    # core/MOM_variables.F90:273-275 Kv_shear [H Z T-1], :255-261 nkml_visc_u [nondim]; parameterizations/vertical/MOM_vert_friction.F90:99 a_u
    # [H T-1], :103 h_u [H]; forces%taux [R Z L T-2]; visc_rem_u [nondim]; taux_bot [R L Z T-2]
    vertvisc=dict(u=0, v=0, h=1, taux=0, tauy=0, Kv_bbl_u=1, Kv_bbl_v=1, bbl_thick_u=0, bbl_thick_v=0, Kv_shear=1, Ray_u=1, Ray_v=1, nkml_visc_u=0,
                  nkml_visc_v=0, ustar=0, visc_rem_u=0, visc_rem_v=0, taux_bot=0, tauy_bot=0, ntrunc=0, a_u=1, a_v=1, h_u=1, h_v=1),
    # core/MOM_continuity_PPM.F90: h, hin [H], uh, vh [H L2 T-1]
    continuity=dict(u=0, v=0, h=1, hn=1, uh=1, vh=1),
    # core/MOM_CoriolisAdv.F90: h [H], uh, vh [H L2 T-1], CAu, CAv [L T-2]
    coradcalc=dict(u=0, v=0, h=1, uh=1, vh=1, CAu=0, CAv=0),
    # core/MOM_PressureForce_FV.F90: h [H], PFu, PFv [L T-2], pbce [L2 T-2 H-1], eta [H]; the non-Boussinesq form the same with H ~> kg m-2
    pressureforce=dict(h=1, T=0, S=0, PFu=0, PFv=0, pbce=-1, eta=1),
    pressureforce_nonbouss=dict(h=1, T=0, S=0, PFu=0, PFv=0, pbce=-1, eta=1),
    # ALE/MOM_ALE.F90:484-492 h, h_new, dzRegrid [H]; :870-875 h_u, h_v [H]; ALE/MOM_regridding.F90:519 coordinateResolution of z* [Z], :571 MIN_THICKNESS
    # scale=GV%m_to_H, :2303-2304 depth_of_time_filter_shallow, _deep [H] (the three options go in as metres times GV%Z_to_H)
    ale_zstar=dict(h=1, u=0, v=0, res=0, h_new=1, dz=1, h_old_u=1, h_old_v=1, h_new_u=1, h_new_v=1, h_dz_u=1, h_dz_v=1),
    # diagnostics/MOM_sum_output.F90:490-760: the totals in kg, J, kg salt ... ; GV%H_to_kg_m2 (MOM_verticalGrid.F90:192) is the argument / 2^c;
    # :326 PE [J], :329-330 Z_0APE [Z ~> m], :691 toten
    sum_output=dict(h=1, u=0, v=0, T=0, S=0, **{n: 0 for n in ("mass_tot", "KE_tot", "PE_tot", "toten", "Salt", "Heat", "max_CFL", "mass_EFP", "salt_EFP",
                                                                "heat_EFP", "npoints", "mass_lay", "KE_lay", "PE", "Z_0APE")}),
)


# ---- the operators of tests/test_properties.py in the shape of the rotation file's registry ------------------------------------------------------------
def hip_ops(dg, g):
    ops = tp.HipOps()
    ops.dgs[id(g)] = dg
    return ops


class Continuity:
    SETS = {"PPM": {}}

    @staticmethod
    def build(ni, nj, topo):
        g, d = tp.case(ni, nj, reentrant=topo)
        return g, dict(u=d["u"], v=d["v"], h=d["h"])

    @staticmethod
    def oracle(g, inp, opt, ops=tp.OracleOps):
        hn, uh, vh = ops.continuity(g, inp["u"], inp["v"], inp["h"], 900.0)
        return dict(hn=hn, uh=uh, vh=vh)

    @classmethod
    def hip(cls, dev, dg, g, inp, opt):
        return cls.oracle(g, inp, opt, hip_ops(dg, g))

    @staticmethod
    def worked(g, inp, out):
        return np.abs(dom(g, out["uh"])).max() > 0 and np.abs(dom(g, out["vh"])).max() > 0 and not np.array_equal(dom(g, out["hn"]), dom(g, inp["h"]))


class CorAdCalc:
    SETS = {s: dict(coriolis_scheme=s) for s in ("SADOURNY75_ENERGY", "ARAKAWA_HSU90", "SADOURNY75_ENSTRO", "ARAKAWA_LAMB81", "ARAKAWA_LAMB_BLEND", "ROBUST_ENSTRO")}

    @staticmethod
    def build(ni, nj, topo):
        g, d = tp.case(ni, nj, reentrant=topo)
        _, uh, vh = tp.OracleOps.continuity(g, d["u"], d["v"], d["h"], 900.0)
        orc.halo_update(g, uh, U); orc.halo_update(g, vh, V)
        return g, dict(u=d["u"], v=d["v"], h=d["h"], uh=uh, vh=vh)

    @staticmethod
    def oracle(g, inp, opt, ops=tp.OracleOps):
        CAu, CAv = ops.coradcalc(g, inp["u"], inp["v"], inp["h"], inp["uh"], inp["vh"], **opt)
        return dict(CAu=CAu, CAv=CAv)

    @classmethod
    def hip(cls, dev, dg, g, inp, opt):
        return cls.oracle(g, inp, opt, hip_ops(dg, g))

    @staticmethod
    def worked(g, inp, out):
        return np.abs(dom(g, out["CAu"])).max() > 0 and np.abs(dom(g, out["CAv"])).max() > 0


class PressureForceBouss:
    SETS = {"wright": {}}

    @staticmethod
    def build(ni, nj, topo):
        g, d = tp.case(ni, nj, reentrant=topo)
        return g, dict(h=d["h"], T=d["T"], S=d["S"])

    @staticmethod
    def oracle(g, inp, opt, ops=tp.OracleOps):
        return dict(zip(("PFu", "PFv", "pbce", "eta"), ops.pressureforce(g, inp["h"], inp["T"], inp["S"])[:4]))

    @classmethod
    def hip(cls, dev, dg, g, inp, opt):
        return cls.oracle(g, inp, opt, hip_ops(dg, g))

    @staticmethod
    def worked(g, inp, out):
        return all(np.abs(dom(g, out[n])).max() > 0 for n in ("PFu", "PFv", "pbce", "eta"))


class PressureForceNonBouss:
    """PressureForce_FV_nonBouss: thicknesses in kg m-2 times 2^c, GV%H_to_RZ = 2^-c (its argument: the grid's H_to_Z times the unit run's 1)"""
    SETS = {"wright": {}}

    @staticmethod
    def build(ni, nj, topo):
        g, d = tp.case(ni, nj, reentrant=topo)
        return g, dict(h=np.ascontiguousarray(d["h"] * g.Rho0), T=d["T"], S=d["S"])

    @staticmethod
    def oracle(g, inp, opt):
        return dict(zip(("PFu", "PFv", "pbce", "eta"), orc.pressureforce_nonbouss(g, orc.pressureforce_cs(g), orc.eos("WRIGHT"), inp["h"], inp["T"], inp["S"],
                                                                                  H_to_RZ=g.H_to_Z)))

    @staticmethod
    def hip(dev, dg, g, inp, opt):
        from mom6_amd.pressure_force import EOS_init, PressureForce, PressureForce_init
        X, N = dev.X, dev.N
        o = dict(PFu=X(g.zeros3(U)), PFv=X(g.zeros3(V)), pbce=X(g.zeros3(H)), eta=X(g.zeros2(H)))
        PressureForce(X(inp["h"]), (X(inp["T"]), X(inp["S"]), EOS_init("WRIGHT")), o["PFu"], o["PFv"], dg, PressureForce_init(g), pbce=o["pbce"], eta=o["eta"],
                      Boussinesq=False, H_to_RZ=g.H_to_Z)
        dg.sync()
        return {n: N(a) for n, a in o.items()}

    worked = PressureForceBouss.worked


class ALEZstar:
    """z* regridding, the velocity-point thicknesses by both routes and the velocity remap of tests/test_regridding.py"""
    SETS = {"default": dict(), "time_filter": dict(old_grid_weight=0.4, zs=50.0, zd=400.0), "min_thickness_0": dict(min_thickness=0.0)}

    @staticmethod
    def build(ni, nj, topo):
        g, d, res = treg.make(ni, nj, reentrant_x=topo[0], reentrant_y=topo[1])
        return g, dict(h=d["h"], u=d["u"], v=d["v"], res=res)

    @staticmethod
    def options(g, opt):
        return dict(min_thickness=opt.get("min_thickness", 1.0e-3) * g.Z_to_H, old_grid_weight=opt.get("old_grid_weight", 0.0), zs=opt.get("zs", 0.0) * g.Z_to_H,
                    zd=opt.get("zd", 0.0) * g.Z_to_H)

    @classmethod
    def oracle(cls, g, inp, opt):
        h_new, dz = orc.ale_regrid(g, orc.regridding_cs(inp["res"], **cls.options(g, opt)), inp["h"])
        orc.halo_update(g, h_new, H)
        o = dict(h_new=h_new, dz=dz, u=inp["u"].copy(), v=inp["v"].copy())
        o["h_old_u"], o["h_old_v"] = orc.ale_remap_set_h_vel(g, inp["h"]); o["h_new_u"], o["h_new_v"] = orc.ale_remap_set_h_vel(g, h_new)
        o["h_dz_u"], o["h_dz_v"] = orc.ale_remap_set_h_vel_via_dz(g, inp["h"], dz)
        orc.ale_remap_velocities(g, "PPM_H4", o["h_old_u"], o["h_old_v"], o["h_new_u"], o["h_new_v"], o["u"], o["v"])
        return o

    @classmethod
    def hip(cls, dev, dg, g, inp, opt):
        from mom6_amd.ale import ALE_regrid, ALE_remap_set_h_vel, ALE_remap_set_h_vel_via_dz, ALE_remap_velocities, initialize_regridding, initialize_remapping
        X, N = dev.X, dev.N
        k = cls.options(g, opt)
        CS = initialize_regridding(dg, coordinateResolution=inp["res"], min_thickness=k["min_thickness"], old_grid_weight=k["old_grid_weight"],
                                   depth_of_time_filter_shallow=k["zs"], depth_of_time_filter_deep=k["zd"])
        h = X(inp["h"])
        o = dict(h_new=X(np.zeros_like(inp["h"])), dz=X(np.zeros((g.nk + 1,) + g.shape2(H))), u=X(inp["u"]), v=X(inp["v"]))
        o.update({f"h_{a}_{b}": X(np.zeros_like(inp[b])) for a in ("old", "new", "dz") for b in ("u", "v")})
        ALE_regrid(dg, h, o["h_new"], o["dz"], None, CS)
        dg.sync()
        h_new = N(o["h_new"]); orc.halo_update(g, h_new, H); o["h_new"] = X(h_new)      # (the pass_var between the two calls in the step)
        ALE_remap_set_h_vel(None, dg, h, o["h_old_u"], o["h_old_v"]); ALE_remap_set_h_vel(None, dg, o["h_new"], o["h_new_u"], o["h_new_v"])
        ALE_remap_set_h_vel_via_dz(None, dg, o["h_new"], o["h_dz_u"], o["h_dz_v"], None, h, o["dz"])
        ALE_remap_velocities(initialize_remapping("PPM_H4"), dg, o["h_old_u"], o["h_old_v"], o["h_new_u"], o["h_new_v"], o["u"], o["v"])
        dg.sync()
        return {n: N(a) for n, a in o.items()}

    @staticmethod
    def worked(g, inp, out):
        return not np.array_equal(dom(g, out["h_new"]), dom(g, inp["h"])) and not np.array_equal(dom(g, out["u"]), dom(g, inp["u"])) and np.abs(dom(g, out["dz"])).max() > 0


class SumOutput:
    """write_energy's mass, energy, salt and heat totals and, with CALCULATE_APE, the available potential energy of each interface, its total and the
    interfaces' reference heights (Z_0APE [Z]): the same numbers in either unit"""
    SETS = {"sums": {}}

    @staticmethod
    def build(ni, nj, topo):
        g, d = tp.case(ni, nj, reentrant=topo)
        return g, {n: d[n] for n in ("u", "v", "h", "T", "S")}

    @staticmethod
    def oracle(g, inp, opt):
        r = orc.write_energy_sums(g, inp["u"], inp["v"], inp["h"], inp["T"], inp["S"], 900.0, H_to_kg_m2=g.Rho0 * g.H_to_Z)
        r.update(orc.write_energy_ape(g, inp["h"], r["mass_lay"], tso.g_prime_of(g.nk), Rho0=g.Rho0, H_to_kg_m2=g.Rho0 * g.H_to_Z))      # CALCULATE_APE :610-680
        r["toten"] = r["KE_tot"] + r["PE_tot"]      # :691
        return SumOutput.plain(r)

    @staticmethod
    def plain(r):
        return {n: tuple(x) if isinstance(x, list) else x for n, x in r.items()}      # (lists of numbers: compared as values, not as fields)

    @staticmethod
    def hip(dev, dg, g, inp, opt):
        from mom6_amd.sum_output import depth_list_setup, write_energy
        X = dev.X
        depth_list_setup(dg)
        return SumOutput.plain(write_energy(X(inp["u"]), X(inp["v"]), X(inp["h"]), (X(inp["T"]), X(inp["S"])), dg, 900.0, H_to_kg_m2=g.Rho0 * g.H_to_Z,
                                            g_prime=tso.g_prime_of(g.nk), Rho0=g.Rho0))

    @staticmethod
    def worked(g, inp, out):
        return out["mass_tot"] > 0 and out["KE_tot"] > 0 and out["Heat"] != 0 and out["npoints"] > 0 and out["PE_tot"] > 0 and out["toten"] > out["KE_tot"] \
            and any(z != 0 for z in out["Z_0APE"])


OPS = dict(trp.OPS, ale_zstar=ALEZstar, sum_output=SumOutput, continuity=Continuity, coradcalc=CorAdCalc, pressureforce=PressureForceBouss, pressureforce_nonbouss=PressureForceNonBouss)
assert set(OPS) == set(DIMS)
# the option sets with an entry that does not scale on the oracle, and those entries: none.  (The reference's own test.dim.h passes; an
# entry that does not scale is a misplaced factor here until the reference's expression shows otherwise.)
EXCEPTIONS = {}
assert len(EXCEPTIONS) <= 3


def build(opname, ni, nj, opt, size=None):
    op = OPS[opname]
    return trp.build(op, ni, nj, TOPO, size or {}, opt) if opname in trp.OPS else op.build(ni, nj, TOPO)


def unchecked(opname, setname):
    return opname == "hor_visc" and setname in trp.HorVisc.UNCHECKED


def test_rescaled_grid_is_the_reference_vertical_grid():
    """verticalGridInit with H_TO_M = 2^-c (MOM_verticalGrid.F90:171-174, :192-221), and the constructor's H_subroundoff for any Z_to_H (:215)"""
    from mom6_amd.grid import Grid
    g, _ = tp.case()
    for c in POWERS + (40,):      # (at 2^40 GV%m_to_H*1e-17 is no longer the smaller argument of the max for ANGSTROM = 0)
        r = rescale_grid(g, c)
        m_to_H = 2.0 ** c
        assert (r.Z_to_H, r.H_to_Z, r.Angstrom_H) == (m_to_H, 1.0 / m_to_H, m_to_H * 1.0e-10)
        assert r.H_subroundoff == 1e-20 * max(r.Angstrom_H, m_to_H * 1e-17) and r.dZ_subroundoff == g.dZ_subroundoff == 1e-20 * max(1.0e-10, 1e-17)
        assert (r.g_Earth, r.Rho0, r.halo, r.first_direction, r.reentrant_x, r.reentrant_y) == (g.g_Earth, g.Rho0, g.halo, g.first_direction, g.reentrant_x, g.reentrant_y)
        assert r.Rho0 * r.H_to_Z == g.Rho0 / m_to_H and r.Z_to_H / r.Rho0 == m_to_H / g.Rho0      # GV%H_to_RZ, GV%RZ_to_H as the library forms them
        assert all(np.array_equal(r.metrics[n], g.metrics[n]) for n in g.metrics) and set(r.metrics) == set(g.metrics)
        z = Grid(ni=4, nj=4, nk=1, Angstrom_H=0.0, Z_to_H=m_to_H, H_to_Z=1.0 / m_to_H)
        assert z.H_subroundoff == 1e-20 * (m_to_H * 1e-17) and z.dZ_subroundoff == 1e-37
    d = scale_fields(dict(a=np.ones(3), b=[np.ones(2)], s=(3, 0.5), n=None), dict(a=1, b=-1, s=0, n=1), 3)
    assert np.all(d["a"] == 8.0) and np.all(d["b"][0] == 0.125) and d["s"] == (3, 0.5) and d["n"] is None
    with pytest.raises(KeyError):
        scale_fields(dict(x=np.ones(2)), dict(a=1), 3)


# ---- the oracle and the checkers scale with the thickness unit (CPU) ----------------------------------------------------------------------------------
CPU_CASES = [(o, s, c) for o, op in OPS.items() for m, s in enumerate(op.SETS) for c in POWERS if c == POWERS[0] or m == 0]


@pytest.mark.parametrize("opname,setname,c", CPU_CASES, ids=[f"{o}-{s}-{c}" for o, s, c in CPU_CASES])
def test_oracle_scales_with_the_thickness_unit(opname, setname, c):
    op = OPS[opname]; opt = op.SETS[setname]
    g, inp = build(opname, NI, NJ, opt)
    gs, inp_s = rescale_grid(g, c), scale_fields(inp, DIMS[opname], c)
    a = op.oracle(g, inp, opt)
    b = op.oracle(gs, inp_s, opt)
    if not unchecked(opname, setname):
        assert op.worked(g, inp, a) and op.worked(gs, inp_s, b), "the operator left its input as it was"
    bad = differences(g, scale_fields(a, DIMS[opname], c), b, np.array_equal)
    assert set(bad) == EXCEPTIONS.get((opname, setname), set()), bad


# ---- the library scales with the thickness unit (GPU) ----------------------------------------------------------------------------------------------------
GPU_SETS = dict(trp.GPU_SETS, **{o: list(OPS[o].SETS) for o in ("ale_zstar", "sum_output", "continuity", "coradcalc", "pressureforce", "pressureforce_nonbouss")})
GPU_CASES = [(o, s, c) for o, sets in GPU_SETS.items() for m, s in enumerate(sets) for c in POWERS if c == POWERS[0] or m == 0]


@functools.lru_cache(maxsize=None)
def unit_library_run(opname, setname):
    """the case and the library's result in the unit it was built in: one run for both powers (nothing writes to either)"""
    op = OPS[opname]; opt = op.SETS[setname]
    g, inp = build(opname, GPU_NI, GPU_NJ, opt, trp.GPU_SIZE.get(opname))
    dev = Dev()
    try:
        return g, inp, op.hip(dev, dev.dg(g), g, inp, opt)
    finally:
        dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("opname,setname,c", GPU_CASES, ids=[f"{o}-{s}-{c}" for o, s, c in GPU_CASES])
def test_library_scales_with_the_thickness_unit(opname, setname, c):
    """(1) on the scaled grid the library is the oracle (the checker), bit for bit; (2) the library's result on the scaled grid is its result on
    the grid times 2^(c e), with the same statistics"""
    op = OPS[opname]; opt = op.SETS[setname]
    g, inp, a = unit_library_run(opname, setname)
    gs, inp_s = rescale_grid(g, c), scale_fields(inp, DIMS[opname], c)
    want_s = op.oracle(gs, inp_s, opt)
    dev = Dev()
    try:
        b = op.hip(dev, dev.dg(gs), gs, inp_s, opt)
    finally:
        dev.close()
    if not unchecked(opname, setname):
        assert op.worked(g, inp, a) and op.worked(gs, inp_s, b), "the operator left its input as it was"
    bad = differences(gs, want_s, b, bits_equal)
    assert not bad, ("the library is not the oracle on the scaled grid", bad)
    bad = set(differences(g, scale_fields(a, DIMS[opname], c), b, np.array_equal)) - EXCEPTIONS.get((opname, setname), set())
    assert not bad, ("the library does not scale with the thickness unit", sorted(bad))


# ---- the whole split RK2 step: two steps, RK2 and RK2B, inviscid and with both viscosities ----------------------------------------------------
# core/MOM_dynamics_split_RK2.F90:288-330: u, v, u_av [L T-1]; h, h_av [H]; uh, vh [H L2 T-1]; uhtr, vhtr [H L2]; eta, eta_av_out [H]
STEP_DIMS = dict(u=0, v=0, h=1, uh=1, vh=1, uhtr=1, vhtr=1, eta=1, eta_av=1, u_av=0, h_av=1, nstep=0, dtbt=0)
STEP_KV_BBL = 1.0e-3      # visc%Kv_bbl_u [H Z T-1]: times 2^c; visc%bbl_thick_u [Z], the stresses and T, S as they are


@functools.lru_cache(maxsize=None)
def unit_step_case(ni, nj, nk):
    g, d = tp.case(ni=ni, nj=nj, nk=nk, seed=5)
    return (g, {n: d[n] for n in ("u", "v", "h", "T", "S")}) + tp.forcing(g)


def step_case(ni, nj, nk, c):
    g, d, taux, tauy = unit_step_case(ni, nj, nk)
    return g, d, rescale_grid(g, c), scale_fields(d, dict(u=0, v=0, h=1, T=0, S=0), c), taux, tauy


@functools.lru_cache(maxsize=None)
def unit_hip_steps(viscous, rk2b):
    """the library's two steps in the unit of the case: one run for both powers"""
    g, d, taux, tauy = unit_step_case(70, 40, 5)
    return tp.hip_steps(g, d, taux, tauy, 900.0, 2, viscous, rk2b=rk2b)


def oracle_step_fields(st):
    return dict(u=st.u, v=st.v, h=st.h, uh=st.uh, vh=st.vh, uhtr=st.uhtr, vhtr=st.vhtr, eta=st.arrs["eta"], eta_av=st.eta_av, nstep=int(st.bcs.nstep_last),
                dtbt=float(st.bcs.dtbt))


@pytest.mark.parametrize("c", POWERS)
@pytest.mark.parametrize("rk2b", [False, True], ids=["RK2", "RK2B"])
@pytest.mark.parametrize("viscous", [False, True], ids=["inviscid", "viscous"])
def test_oracle_rk2_step_scales_with_the_thickness_unit(viscous, rk2b, c):
    g, d, gs, ds, taux, tauy = step_case(22, 16, 3, c)
    a = oracle_step_fields(tp.oracle_steps(g, d, taux, tauy, 900.0, 2, viscous, rk2b))
    b = oracle_step_fields(tp.oracle_steps(gs, ds, taux, tauy, 900.0, 2, viscous, rk2b, Kv_bbl=STEP_KV_BBL * 2.0 ** c))
    assert np.abs(a["u"]).max() > 0 and a["nstep"] >= 1 and not np.array_equal(interior(g, a["h"]), interior(g, d["h"]))
    bad = differences(g, scale_fields(a, STEP_DIMS, c), b, np.array_equal)
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("c", POWERS)
@pytest.mark.parametrize("rk2b", [False, True], ids=["RK2", "RK2B"])
@pytest.mark.parametrize("viscous", [False, True], ids=["inviscid", "viscous"])
def test_hip_rk2_step_scales_with_the_thickness_unit(viscous, rk2b, c):
    g, d, gs, ds, taux, tauy = step_case(70, 40, 5, c)
    want = oracle_step_fields(tp.oracle_steps(gs, ds, taux, tauy, 900.0, 2, viscous, rk2b, Kv_bbl=STEP_KV_BBL * 2.0 ** c, bound_coriolis=False))
    a = unit_hip_steps(viscous, rk2b)
    b = tp.hip_steps(gs, ds, taux, tauy, 900.0, 2, viscous, rk2b=rk2b, Kv_bbl=STEP_KV_BBL * 2.0 ** c)
    assert np.abs(a["u"]).max() > 0 and a["nstep"] >= 1
    bad = differences(gs, want, {n: b[n] for n in want}, bits_equal)
    assert not bad, ("the library's step is not the oracle's on the scaled grid", bad)
    bad = differences(g, scale_fields(a, STEP_DIMS, c), b, np.array_equal)
    assert not bad, ("the library's step does not scale with the thickness unit", bad)


# ---- btstep with btcalc, bt_mass_source and set_dtbt (tests/test_barotropic.py) --------------------------------------------------------------------
# core/MOM_barotropic.F90:431-500: U_in, U_Cor, u_uh0 [L T-1]; eta_in, eta_PF_in, eta_out, etaav [H]; bc_accel_u, accel_layer_u [L T-2]; pbce
# [L2 T-2 H-1]; taux [R L Z T-2]; visc_rem_u, frhatu (:105) [nondim]; uh0, uhbtav [H L2 T-1]; ubtav (:117) [L T-1]; eta_cor (:129) [H]; dtbt,
# dtbt_max (:163) [T].  BT_cont_type, core/MOM_variables.F90:290-316: FA_u_* [H L], uBT_* [L T-1], h_u [H].
BT_DIMS = dict(U_in=0, V_in=0, eta_in=1, dt=0, bc_accel_u=0, bc_accel_v=0, taux=0, tauy=0, pbce=-1, eta_PF_in=1, U_Cor=0, V_Cor=0, visc_rem_u=0, visc_rem_v=0,
               bt_cont=None, uh0=1, vh0=1, u_uh0=0, v_vh0=0, accel_layer_u=0, accel_layer_v=0, eta_out=1, uhbtav=1, vhbtav=1, etaav=1, ubtav=0, vbtav=0,
               frhatu=0, frhatv=0, eta_cor=1, nstep=0, dtbt=0, dtbt_max=0, h=1, h_u=1, h_v=1,
               **{n: 1 for n in _abi.BT_CONT_U + _abi.BT_CONT_V if n.startswith("FA_")}, **{n: 0 for n in _abi.BT_CONT_U + _abi.BT_CONT_V if "BT_" in n})
BT_SETS = {"bt_cont": dict(), "bt_cont_strong_drag": dict(strong_drag=1), "linear_areas": dict(use_bt_cont=False), "linear_areas_strong_drag": dict(use_bt_cont=False, strong_drag=1),
           "nonlinear_areas": dict(use_bt_cont=False, Nonlinear_continuity=1)}
BT_CASES = [(s, c) for m, s in enumerate(BT_SETS) for c in POWERS if c == POWERS[0] or m == 0]


def oracle_btstep(kw):
    """the oracle's btstep on barotropic_case(**kw): the grid, every input (BT_cont and h among them) and every result"""
    g, cs, case, keep = barotropic_case(orc, **kw)
    out = tbt.run_oracle(g, cs, case, want_etaav=True)
    out.update({n: keep["cs_arrs"][n] for n in ("ubtav", "vbtav", "frhatu", "frhatv", "eta_cor")}, nstep=int(cs.nstep_last), dtbt=float(cs.dtbt), dtbt_max=float(cs.dtbt_max))
    return g, dict({n: a for n, a in case.items() if n != "bt_cont"}, h=keep["h"], **keep["bt_arrs"]), out


@pytest.mark.parametrize("setname,c", BT_CASES, ids=[f"{s}-{c}" for s, c in BT_CASES])
def test_oracle_btstep_scales_with_the_thickness_unit(setname, c):
    kw = dict(BT_SETS[setname], ni=NI, nj=NJ)
    g, inp, a = oracle_btstep(kw)
    gs, inp_s, b = oracle_btstep(dict(kw, H_power=c))
    assert a["nstep"] > 3 and np.abs(dom(g, a["uhbtav"])).max() > 0 and not np.array_equal(dom(g, a["eta_out"]), dom(g, inp["eta_in"]))
    # the scaled case is the unit case in the other unit: continuity's BT_cont and fluxes, the pressure force's pbce and eta_PF
    bad = differences(g, scale_fields(inp, BT_DIMS, c), inp_s, np.array_equal)
    assert not bad, ("inputs", bad)
    bad = differences(g, scale_fields(a, BT_DIMS, c), b, np.array_equal)
    assert not bad, bad


@functools.lru_cache(maxsize=None)
def unit_btstep(setname):
    return tbt.btstep_against_the_oracle(dict(BT_SETS[setname], ni=GPU_NI, nj=GPU_NJ))


@pytest.mark.gpu
@pytest.mark.parametrize("setname,c", BT_CASES, ids=[f"{s}-{c}" for s, c in BT_CASES])
def test_library_btstep_scales_with_the_thickness_unit(setname, c):
    """on the scaled grid barotropic_init, btcalc, bt_mass_source, set_dtbt and btstep are the oracle's, bit for bit (the assertions of
    test_btstep_matches_oracle_bitwise); the library's results scale"""
    kw = dict(BT_SETS[setname], ni=GPU_NI, nj=GPU_NJ)
    g, _, _, a = unit_btstep(setname)
    gs, _, _, b = tbt.btstep_against_the_oracle(dict(kw, H_power=c))
    assert a["nstep"] >= 1 and np.abs(dom(g, a["uhbtav"])).max() > 0      # (nonlinear_areas: one step, as in test_btstep_matches_oracle_bitwise)
    bad = differences(g, scale_fields(a, BT_DIMS, c), b, np.array_equal)
    assert not bad, ("the library's btstep does not scale with the thickness unit", bad)


def test_thickness_diffuse_refuses_a_record_set_up_without_a_grid():
    """KD_SMOOTH becomes [H Z T-1] with the grid's Z_to_H (MOM_thickness_diffuse.F90:2304): a record of thickness_diffuse_init(None, ...) can be
    looked at, not run"""
    from mom6_amd._lib import Mom6HipError
    from mom6_amd.thickness_diffuse import thickness_diffuse, thickness_diffuse_init
    g, _ = tp.case()
    assert thickness_diffuse_init(rescale_grid(g, 11), KHTH=100.0, KD_SMOOTH=1.0e-6).st.kappa_smooth == 1.0e-6 * 2.0 ** 11
    CS = thickness_diffuse_init(None, THICKNESSDIFFUSE=True, KHTH=100.0)
    with pytest.raises(Mom6HipError, match="no grid"):
        thickness_diffuse(None, None, None, None, 900.0, None, None, None, None, CS)
