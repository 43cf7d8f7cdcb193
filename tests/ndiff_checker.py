"""A plain-Python restatement of the neutral branch of tracer_hordiff (src/tracer/MOM_tracer_hor_diff.F90:474-534) with the continuous
reconstruction of src/tracer/MOM_neutral_diffusion.F90, in the reference's order of operations on Python floats (IEEE fp64):
neutral_diffusion_calc_coeffs (:337) with NDIFF_INTERIOR_ONLY, compute_tapering_coeffs (:1022, NDIFF_TAPERING), the interface
coefficients of KHTR_USE_EBT_STRUCT (MOM_tracer_hor_diff.F90:489-518) and Coef_h (:670-684), neutral_surface_flux with coefficients
(:2297) and the update of the tracers (:834-924).  With both switches off it is orc.tracer_hordiff(..., neutral=...) bit for bit
(tests/test_ndiff_taper_ebt.py), which ties this text to the oracle and through it to the reference's own unit-test answers.

What the oracle exports is called, not restated: interface_scalar, the density derivatives of the equation of state, the halo update and
interpolate_for_nondim_position."""
import math

import numpy as np

from hbd_checker import SURFACE, boundary_k_range, khdt_and_itts, max2, min2
from mom6_amd import _abi
from oracle import orc


def signum(a, x):
    """:1200"""
    return 0. if x == 0. else math.copysign(abs(a), x)


def fsign(a, b):
    return math.copysign(abs(a), b)


def ppm_left_right_edge_values(nk, Tl, Ti):
    """:2541"""
    aL, aR = [0.0] * nk, [0.0] * nk
    for k in range(nk):
        aL[k] = Ti[k]; aR[k] = Ti[k + 1]
        if signum(1., aR[k] - Tl[k]) * signum(1., Tl[k] - aL[k]) <= 0.0:
            aL[k] = Tl[k]; aR[k] = Tl[k]
        elif fsign(3., aR[k] - aL[k]) * ((Tl[k] - aL[k]) + (Tl[k] - aR[k])) > abs(aR[k] - aL[k]):
            aL[k] = Tl[k] + 2.0 * (Tl[k] - aR[k])
        elif fsign(3., aR[k] - aL[k]) * ((Tl[k] - aL[k]) + (Tl[k] - aR[k])) < -abs(aR[k] - aL[k]):
            aR[k] = Tl[k] + 2.0 * (Tl[k] - aL[k])
    return aL, aR


def ppm_ave(xL, xR, aL, aR, aMean):
    """:1166"""
    dx = xR - xL
    xave = 0.5 * (xR + xL)
    a6o3 = 2. * aMean - (aL + aR)
    a6 = 3. * a6o3
    if dx < 0. or dx > 1.:
        raise RuntimeError("ppm_ave: dx<0 or dx>1 should not happened!")
    if dx == 0.:
        return aL + (aR - aL) * xR + a6 * xR * (1. - xR)
    return (aL + xave * ((aR - aL) + a6)) - a6o3 * (xR * xR + xR * xL + xL * xL)


def find_neutral_surface_positions_continuous(nk, Pl, Tl, Sl, dRdTl, dRdSl, Pr, Tr, Sr, dRdTr, dRdSr, bl=None):
    """:1353 -> PoL, PoR, KoL, KoR (1-based), hEff; bl = (bl_kl, bl_kr, bl_zl, bl_zr): the boundary-layer limits of :1508-1521"""
    ns = 2 * nk + 2
    PoL, PoR, KoL, KoR, hEff = [0.0] * ns, [0.0] * ns, [1] * ns, [1] * ns, [0.0] * (ns - 1)
    kr = kl = lastK_right = lastK_left = 1
    lastP_right = lastP_left = 0.
    reached_bottom = searching_left = searching_right = False
    L = lambda a, k: a[k - 1]
    ifndp = orc.ndiff_ifndp

    def absolute_position(Pint, Karr, NParr, ks):
        k = Karr[ks] - 1
        return Pint[k] + NParr[ks] * (Pint[k + 1] - Pint[k])

    for ks in range(ns):
        klm1 = max(kl - 1, 1)
        krm1 = max(kr - 1, 1)
        dRho = 0.5 * ((L(dRdTr, kr) + L(dRdTl, kl)) * (L(Tr, kr) - L(Tl, kl)) + (L(dRdSr, kr) + L(dRdSl, kl)) * (L(Sr, kr) - L(Sl, kl)))
        if not reached_bottom:
            if dRho < 0.:
                searching_left, searching_right = True, False
            elif dRho > 0.:
                searching_right, searching_left = True, False
            elif kl + kr == 2:
                searching_left, searching_right = True, False
            else:
                searching_left, searching_right = not searching_left, not searching_right
        if searching_left:
            dRhoTop = 0.5 * ((L(dRdTl, klm1) + L(dRdTr, kr)) * (L(Tl, klm1) - L(Tr, kr)) + (L(dRdSl, klm1) + L(dRdSr, kr)) * (L(Sl, klm1) - L(Sr, kr)))
            dRhoBot = 0.5 * ((L(dRdTl, klm1 + 1) + L(dRdTr, kr)) * (L(Tl, klm1 + 1) - L(Tr, kr)) +
                             (L(dRdSl, klm1 + 1) + L(dRdSr, kr)) * (L(Sl, klm1 + 1) - L(Sr, kr)))
            if dRhoTop > 0. or kr + kl == 2:
                PoL[ks] = 0.
            elif dRhoTop >= dRhoBot:
                PoL[ks] = 1.
            else:
                PoL[ks] = ifndp(dRhoTop, L(Pl, klm1), dRhoBot, L(Pl, klm1 + 1))
            if PoL[ks] >= 1. and klm1 < nk:
                klm1 = klm1 + 1
                PoL[ks] = PoL[ks] - 1.
            if float(klm1 - lastK_left) + (PoL[ks] - lastP_left) < 0.:
                PoL[ks] = lastP_left
                klm1 = lastK_left
            KoL[ks] = klm1
            if kr <= nk:
                PoR[ks] = 0.; KoR[ks] = kr
            else:
                PoR[ks] = 1.; KoR[ks] = nk
            if kr <= nk:
                kr = kr + 1
            else:
                reached_bottom, searching_right, searching_left = True, True, False
        else:
            dRhoTop = 0.5 * ((L(dRdTr, krm1) + L(dRdTl, kl)) * (L(Tr, krm1) - L(Tl, kl)) + (L(dRdSr, krm1) + L(dRdSl, kl)) * (L(Sr, krm1) - L(Sl, kl)))
            dRhoBot = 0.5 * ((L(dRdTr, krm1 + 1) + L(dRdTl, kl)) * (L(Tr, krm1 + 1) - L(Tl, kl)) +
                             (L(dRdSr, krm1 + 1) + L(dRdSl, kl)) * (L(Sr, krm1 + 1) - L(Sl, kl)))
            if dRhoTop >= 0. or kr + kl == 2:
                PoR[ks] = 0.
            elif dRhoTop >= dRhoBot:
                PoR[ks] = 1.
            else:
                PoR[ks] = ifndp(dRhoTop, L(Pr, krm1), dRhoBot, L(Pr, krm1 + 1))
            if PoR[ks] >= 1. and krm1 < nk:
                krm1 = krm1 + 1
                PoR[ks] = PoR[ks] - 1.
            if float(krm1 - lastK_right) + (PoR[ks] - lastP_right) < 0.:
                PoR[ks] = lastP_right
                krm1 = lastK_right
            KoR[ks] = krm1
            if kl <= nk:
                PoL[ks] = 0.; KoL[ks] = kl
            else:
                PoL[ks] = 1.; KoL[ks] = nk
            if kl <= nk:
                kl = kl + 1
            else:
                reached_bottom, searching_right, searching_left = True, False, True
        if bl is not None:
            bl_kl, bl_kr, bl_zl, bl_zr = bl
            if KoL[ks] <= bl_kl:
                KoL[ks] = bl_kl
                if PoL[ks] < bl_zl:
                    PoL[ks] = bl_zl
            if KoR[ks] <= bl_kr:
                KoR[ks] = bl_kr
                if PoR[ks] < bl_zr:
                    PoR[ks] = bl_zr
        lastK_left, lastP_left, lastK_right, lastP_right = KoL[ks], PoL[ks], KoR[ks], PoR[ks]
        if ks > 0:
            hL = absolute_position(Pl, KoL, PoL, ks) - absolute_position(Pl, KoL, PoL, ks - 1)
            hR = absolute_position(Pr, KoR, PoR, ks) - absolute_position(Pr, KoR, PoR, ks - 1)
            hEff[ks - 1] = 2. * hL * hR / (hL + hR) if hL + hR > 0. else 0.
    return PoL, PoR, KoL, KoR, hEff


def compute_tapering_coeffs(ne, bld_l, bld_r, h_l, h_r):
    """:1022-1075 -> coeff_l, coeff_r (ne values each; entry K-1 is interface K) and (k_min_l, k_max_l, k_min_r, k_max_r)"""
    coeff_l, coeff_r = [1.0] * ne, [1.0] * ne
    max_bld = max2(bld_l, bld_r)
    min_bld = min2(bld_l, bld_r)
    k_min_l = boundary_k_range(SURFACE, ne - 1, h_l, min_bld)[2]
    k_min_r = boundary_k_range(SURFACE, ne - 1, h_r, min_bld)[2]
    k_max_l = boundary_k_range(SURFACE, ne - 1, h_l, max_bld)[2]
    k_max_r = boundary_k_range(SURFACE, ne - 1, h_r, max_bld)[2]
    for k in range(1, k_min_l + 1):
        coeff_l[k - 1] = 0.0
    for k in range(k_min_l + 1, k_max_l + 2):
        coeff_l[k - 1] = (float(k - k_min_l) + 1.0) / (float(k_max_l - k_min_l) + 2.0)
    for k in range(1, k_min_r + 1):
        coeff_r[k - 1] = 0.0
    for k in range(k_min_r + 1, k_max_r + 2):
        coeff_r[k - 1] = (float(k - k_min_r) + 1.0) / (float(k_max_r - k_min_r) + 2.0)
    return coeff_l, coeff_r, (k_min_l, k_max_l, k_min_r, k_max_r)


def neutral_surface_flux(nk, hl, hr, Tl, Tr, PiL, PiR, KoL, KoR, hEff, h_neglect, coeff_l=None, coeff_r=None):
    """:2297, continuous -> Flx (2nk+1 values); KoL, KoR 1-based"""
    nsurf = 2 * nk + 2
    tapering = coeff_l is not None and coeff_r is not None
    khtr_ave = 1.0
    Til = [float(x) for x in orc.ndiff_interface_scalar(hl, Tl, 2, h_neglect)]
    Tir = [float(x) for x in orc.ndiff_interface_scalar(hr, Tr, 2, h_neglect)]
    aL_l, aR_l = ppm_left_right_edge_values(nk, Tl, Til)
    aL_r, aR_r = ppm_left_right_edge_values(nk, Tr, Tir)
    Flx = [0.0] * (nsurf - 1)
    for ks in range(nsurf - 1):
        if hEff[ks] == 0.:
            Flx[ks] = 0.
            continue
        klb, klt, krb, krt = KoL[ks + 1], KoL[ks], KoR[ks + 1], KoR[ks]      # 1-based
        if tapering:
            khtr_ave = 0.25 * ((coeff_l[klb - 1] + coeff_l[klt - 1]) + (coeff_r[krb - 1] + coeff_r[krt - 1]))
        T_left_bottom = (1. - PiL[ks + 1]) * Til[klb - 1] + PiL[ks + 1] * Til[klb]
        T_left_top = (1. - PiL[ks]) * Til[klt - 1] + PiL[ks] * Til[klt]
        T_left_layer = ppm_ave(PiL[ks], PiL[ks + 1] + float(klb - klt), aL_l[klt - 1], aR_l[klt - 1], Tl[klt - 1])
        T_right_bottom = (1. - PiR[ks + 1]) * Tir[krb - 1] + PiR[ks + 1] * Tir[krb]
        T_right_top = (1. - PiR[ks]) * Tir[krt - 1] + PiR[ks] * Tir[krt]
        T_right_layer = ppm_ave(PiR[ks], PiR[ks + 1] + float(krb - krt), aL_r[krt - 1], aR_r[krt - 1], Tr[krt - 1])
        dT_top = T_right_top - T_left_top
        dT_bottom = T_right_bottom - T_left_bottom
        dT_ave = 0.5 * (dT_top + dT_bottom)
        dT_layer = T_right_layer - T_left_layer
        if signum(1., dT_top) * signum(1., dT_bottom) <= 0. or signum(1., dT_ave) * signum(1., dT_layer) <= 0.:
            dT_ave = 0.
        else:
            dT_ave = dT_layer
        Flx[ks] = dT_ave * hEff[ks] * khtr_ave
    return Flx


# ---- the 3-D routines: Fortran (i,j) of an h-point array is [j-1, i-1], of a u-point array [j-1, I], of a v-point array [J, i-1] --------
def col(a, c):
    return [float(x) for x in a[:, c[0], c[1]]]


def faces(g):
    """(direction, face index, left cell, right cell, wet) of every face the branch visits, as array indices"""
    out = []
    for j in range(g.jsc, g.jec + 1):
        for I in range(g.isc - 1, g.iec + 1):
            out.append((0, (j - 1, I), (j - 1, I - 1), (j - 1, I), g.mask2dCu[j - 1, I] > 0.))
    for J in range(g.jsc - 1, g.jec + 1):
        for i in range(g.isc, g.iec + 1):
            out.append((1, (J, i - 1), (J - 1, i - 1), (J, i - 1), g.mask2dCv[J, i - 1] > 0.))
    return out


class NDCS:
    """neutral_diffusion_CS as neutral_diffusion_init (:138) leaves it, parameters by their reference names"""

    def __init__(self, g, eos, NDIFF_REF_PRES=-1.0, NDIFF_ANSWER_DATE=20240101, NDIFF_INTERIOR_ONLY=False, NDIFF_TAPERING=False,
                 KHTR_USE_EBT_STRUCT=False, H_to_RZ=None):
        self.eos, self.ref_pres, self.ndiff_answer_date = eos, float(NDIFF_REF_PRES), int(NDIFF_ANSWER_DATE)
        self.interior_only = bool(NDIFF_INTERIOR_ONLY)
        self.tapering = bool(NDIFF_TAPERING) and self.interior_only      # read with NDIFF_INTERIOR_ONLY only (:193-198)
        self.KhTh_use_ebt_struct = bool(KHTR_USE_EBT_STRUCT)
        self.H_to_RZ = float(g.Rho0 * g.H_to_Z if H_to_RZ is None else H_to_RZ)
        self.hbl = None
        self.surf = None      # per face: None (dry) or (PoL, PoR, KoL, KoR, hEff)
        self.taper = None     # per face: None or (coeff_l, coeff_r, the four layer numbers)


def neutral_diffusion_calc_coeffs(g, h, T, S, CS, p_surf=None, h_ML=None):
    """:337-602"""
    nk = g.nk
    h_neglect = g.H_subroundoff
    pa_to_H = 1. / (CS.H_to_RZ * g.g_Earth)
    k_bot, zeta_bot = {}, {}
    if CS.interior_only:
        if h_ML is None:
            raise RuntimeError("hor_bnd_diffusion requires that visc%h_ML is associated.")
        CS.hbl = np.array(h_ML, dtype=np.float64)
        orc.halo_update(g, CS.hbl, _abi.POS_H)
    cols = {}
    for j in range(g.jsc - 1, g.jec + 2):
        for i in range(g.isc - 1, g.iec + 2):
            c = (j - 1, i - 1)
            hc, Tc, Sc = col(h, c), col(T, c), col(S, c)
            k_bot[c], zeta_bot[c] = 1, 0.
            if CS.interior_only and g.mask2dT[c] > 0.:
                _, _, k_bot[c], zeta_bot[c] = boundary_k_range(SURFACE, nk, hc, float(CS.hbl[c]))
            P = [0.0] * (nk + 1)
            P[0] = float(p_surf[c]) if p_surf is not None else 0.
            for k in range(nk):
                P[k + 1] = P[k] + hc[k] * (g.g_Earth * CS.H_to_RZ)
            Ti = [float(x) for x in orc.ndiff_interface_scalar(hc, Tc, 2, h_neglect)]
            Si = [float(x) for x in orc.ndiff_interface_scalar(hc, Sc, 2, h_neglect)]
            dRdT, dRdS = [0.0] * (nk + 1), [0.0] * (nk + 1)
            for K in range(nk + 1):
                dRdT[K], dRdS[K] = orc.eos_density_derivs(CS.eos, Ti[K], Si[K], CS.ref_pres if CS.ref_pres >= 0. else P[K])
            cols[c] = (P, Ti, Si, dRdT, dRdS)
    CS.surf, CS.taper = [], []
    for d, f, cL, cR, wet in faces(g):
        if not wet:
            CS.surf.append(None); CS.taper.append(None)
            continue
        bl = (k_bot[cL], k_bot[cR], zeta_bot[cL], zeta_bot[cR]) if CS.interior_only else None
        PoL, PoR, KoL, KoR, hEff = find_neutral_surface_positions_continuous(nk, *cols[cL], *cols[cR], bl=bl)
        CS.surf.append((PoL, PoR, KoL, KoR, [x * pa_to_H for x in hEff]))      # :570-575
        CS.taper.append(compute_tapering_coeffs(nk + 1, float(CS.hbl[cL]), float(CS.hbl[cR]), col(h, cL), col(h, cR))
                        if CS.tapering else None)


def interface_coefficients(g, khdt_x, khdt_y, I_numitts, ebt_struct=None, KhTr_min=None):
    """Coef_x, Coef_y at the nk+1 interfaces (MOM_tracer_hor_diff.F90:414-462 for HBD, :489-518 for neutral diffusion) as arrays
    [nk+1][u points], [nk+1][v points].  ebt_struct: VarMix%ebt_struct with KHTR_USE_EBT_STRUCT; KhTr_min: the floor of
    FULL_DEPTH_KHTR_MIN (the HBD branch only), compared as the reference writes it"""
    nk = g.nk
    Coef_x, Coef_y = np.zeros((nk + 1,) + g.shape2(_abi.POS_U)), np.zeros((nk + 1,) + g.shape2(_abi.POS_V))
    for j in range(g.jsc, g.jec + 1):
        for I in range(g.isc - 1, g.iec + 1):
            c1 = I_numitts * float(khdt_x[j - 1, I])
            for K in range(1, nk + 2):
                c = c1
                if ebt_struct is not None and K >= 2:
                    c = c1 * 0.5 * (float(ebt_struct[K - 2, j - 1, I - 1]) + float(ebt_struct[K - 2, j - 1, I]))
                    if KhTr_min is not None:
                        c = max2(c, KhTr_min)
                Coef_x[K - 1, j - 1, I] = c
    for J in range(g.jsc - 1, g.jec + 1):
        for i in range(g.isc, g.iec + 1):
            c1 = I_numitts * float(khdt_y[J, i - 1])
            for K in range(1, nk + 2):
                c = c1
                if ebt_struct is not None and K >= 2:
                    c = c1 * 0.5 * (float(ebt_struct[K - 2, J - 1, i - 1]) + float(ebt_struct[K - 2, J, i - 1]))
                    if KhTr_min is not None:
                        c = max2(c, KhTr_min)
                Coef_y[K - 1, J, i - 1] = c
    return Coef_x, Coef_y


def coef_h(g, Coef_x, Coef_y):
    """:670-684: Coef_x and Coef_y averaged at the wet h points of the compute domain, zero elsewhere, then pass_var"""
    nk = g.nk
    Ch = np.zeros((nk + 1,) + g.shape2(_abi.POS_H))
    for j in range(g.jsc, g.jec + 1):
        for i in range(g.isc, g.iec + 1):
            m = float(g.mask2dT[j - 1, i - 1])
            if m > 0.:
                normalize = 1.0 / ((float(g.mask2dCu[j - 1, i - 1]) + float(g.mask2dCu[j - 1, i])) +
                                   (float(g.mask2dCv[j - 1, i - 1]) + float(g.mask2dCv[j, i - 1])) + 1.0e-37)
                for K in range(nk + 1):
                    Ch[K, j - 1, i - 1] = normalize * m * ((float(Coef_x[K, j - 1, i - 1]) + float(Coef_x[K, j - 1, i])) +
                                                           (float(Coef_y[K, j - 1, i - 1]) + float(Coef_y[K, j, i - 1])))
    orc.halo_update(g, Ch, _abi.POS_H)
    return Ch


def neutral_diffusion(g, h, Coef_x, Coef_y, tr, CS, conc_underflow=None):
    """:605-1019 for every tracer of tr (updated in place on the compute domain); Coef_x, Coef_y at the nk+1 interfaces"""
    nk = g.nk
    ns = 2 * nk + 2
    Hs = g.H_subroundoff
    ebt = CS.KhTh_use_ebt_struct
    Ch = coef_h(g, Coef_x, Coef_y) if ebt else None
    fl = faces(g)
    for m, t in enumerate(tr):
        uFlx, vFlx = {}, {}
        for (d, f, cL, cR, wet), surf, tap in zip(fl, CS.surf, CS.taper):
            F = [0.0] * (ns - 1)
            if wet:
                PoL, PoR, KoL, KoR, hEff = surf
                coeff_l = coeff_r = None
                if ebt and CS.tapering:
                    cl, cr = col(Ch, cL), col(Ch, cR)
                    coeff_l = [tap[0][K] * cl[K] for K in range(nk + 1)]
                    coeff_r = [tap[1][K] * cr[K] for K in range(nk + 1)]
                elif ebt:
                    coeff_l, coeff_r = col(Ch, cL), col(Ch, cR)
                elif CS.tapering:
                    coeff_l, coeff_r = tap[0], tap[1]
                F = neutral_surface_flux(nk, col(h, cL), col(h, cR), col(t, cL), col(t, cR), PoL, PoR, KoL, KoR, hEff, Hs, coeff_l, coeff_r)
            (uFlx if d == 0 else vFlx)[f] = (F, surf)
        cu = 0.0 if conc_underflow is None else float(conc_underflow[m])
        new = {}
        for j in range(g.jsc, g.jec + 1):
            for i in range(g.isc, g.iec + 1):
                if not g.mask2dT[j - 1, i - 1] > 0.:
                    continue
                (fE, sE), (fW, sW) = uFlx[(j - 1, i)], uFlx[(j - 1, i - 1)]
                (fN, sN), (fS, sS) = vFlx[(j, i - 1)], vFlx[(j - 1, i - 1)]
                one = [1] * ns
                kE, kW = (sE[2] if sE else one), (sW[3] if sW else one)      # uKoL(I,j,:), uKoR(I-1,j,:)
                kN, kS = (sN[2] if sN else one), (sS[3] if sS else one)      # vKoL(i,J,:), vKoR(i,J-1,:)
                cE = cW = cN = cS = 1.0
                if not ebt:      # Coef_x(I,j,1) ... (:880-905)
                    cE, cW = float(Coef_x[0, j - 1, i]), float(Coef_x[0, j - 1, i - 1])
                    cN, cS = float(Coef_y[0, j, i - 1]), float(Coef_y[0, j - 1, i - 1])
                mul = (lambda c, x: x) if ebt else (lambda c, x: c * x)
                if CS.ndiff_answer_date <= 20240330:
                    dT = [0.0] * nk
                    for ks in range(ns - 1):
                        k = kE[ks] - 1; dT[k] = dT[k] + mul(cE, fE[ks])
                        k = kW[ks] - 1; dT[k] = dT[k] - mul(cW, fW[ks])
                        k = kN[ks] - 1; dT[k] = dT[k] + mul(cN, fN[ks])
                        k = kS[ks] - 1; dT[k] = dT[k] - mul(cS, fS[ks])
                else:
                    dN, dS, dE, dW = [0.0] * nk, [0.0] * nk, [0.0] * nk, [0.0] * nk
                    for ks in range(ns - 1):
                        k = kE[ks] - 1; dE[k] = dE[k] + mul(cE, fE[ks])
                        k = kW[ks] - 1; dW[k] = dW[k] - mul(cW, fW[ks])
                        k = kN[ks] - 1; dN[k] = dN[k] + mul(cN, fN[ks])
                        k = kS[ks] - 1; dS[k] = dS[k] - mul(cS, fS[ks])
                    dT = [(dN[k] + dS[k]) + (dE[k] + dW[k]) for k in range(nk)]
                for k in range(nk):
                    x = float(t[k, j - 1, i - 1]) + dT[k] * (float(g.IareaT[j - 1, i - 1]) / (float(h[k, j - 1, i - 1]) + Hs))
                    if abs(x) < cu:
                        x = 0.0
                    new[(k, j - 1, i - 1)] = x
        for idx, x in new.items():
            t[idx] = x


def tracer_hordiff_neutral(g, h, dt, tr, KhTr, eos, idx_T=0, idx_S=1, max_diff_CFL=-1.0, check_diffusive_CFL=False, conc_underflow=None,
                           p_surf=None, h_ML=None, ebt_struct=None, KhTr_min=0.0, recalc_neutral_surf=False, **nd):
    """the neutral branch of tracer_hordiff (:474-534) with a constant KHTR; tr is updated in place.  ebt_struct: VarMix%ebt_struct, which
    sets KHTR_USE_EBT_STRUCT -- and VarMix%use_variable_mixing, as VarMix_init does, so the diffusivity of a face is
    max(KHTR, KHTR_MIN) (:238-245).  nd: NDIFF_* by their reference names.  Returns (num_itts, halo_updates, max_CFL)"""
    if KhTr <= 0.0 and ebt_struct is None or not tr:
        return 0, 0, 0.0
    CS = NDCS(g, eos, NDIFF_INTERIOR_ONLY=h_ML is not None, KHTR_USE_EBT_STRUCT=ebt_struct is not None, **nd)
    Kh = max2(KhTr, KhTr_min) if ebt_struct is not None else KhTr
    khdt_x, khdt_y, num_itts, I_numitts, max_CFL = khdt_and_itts(g, dt, Kh, max_diff_CFL, check_diffusive_CFL)
    halo_updates = 0
    for t in tr:
        orc.halo_update(g, t, _abi.POS_H)
    halo_updates += 1
    neutral_diffusion_calc_coeffs(g, h, tr[idx_T], tr[idx_S], CS, p_surf, h_ML)
    Coef_x, Coef_y = interface_coefficients(g, khdt_x, khdt_y, I_numitts, ebt_struct)
    for itt in range(1, num_itts + 1):
        if itt > 1:
            for t in tr:
                orc.halo_update(g, t, _abi.POS_H)
            halo_updates += 1
            if recalc_neutral_surf:
                neutral_diffusion_calc_coeffs(g, h, tr[idx_T], tr[idx_S], CS, p_surf, h_ML)
        neutral_diffusion(g, h, Coef_x, Coef_y, tr, CS, conc_underflow)
    return num_itts, halo_updates, max_CFL
