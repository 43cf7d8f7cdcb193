"""The NDIFF_CONTINUOUS = False branch of MOM_neutral_diffusion (src/tracer/MOM_neutral_diffusion.F90) restated in plain Python, one
expression a line as the reference writes them: neutral_diffusion_calc_coeffs (:394-508), mark_unstable_cells (:1841),
find_neutral_surface_positions_discontinuous (:1604) with search_other_column (:1860), find_neutral_pos_linear (:1964),
find_neutral_pos_full (:2084) and calc_delta_rho_and_derivs (:2177), and the discontinuous half of neutral_surface_flux (:2442-2471) with
neutral_surface_T_eval (:2478).  The update of the tracers (:880-914) is ndiff_checker's, with nsurf = 4 nk.  The equation of state and
the reconstructions of src/ALE are the oracle's scalar routines, as ndiff_checker takes them."""
import math

import numpy as np

import ndiff_checker as nc
from hbd_checker import SURFACE, boundary_k_range, khdt_and_itts
from mom6_amd import _abi
from oracle import orc

SCHEMES = ("PLM", "PPM_H4", "PPM_IH4")
FORMS = ("full", "mid_pressure", "local_pressure")


class NegativeThickness(RuntimeError):
    pass


class DiscCS:
    """the part of neutral_diffusion_CS the discontinuous branch reads (:219-277), parameters by their reference names"""

    def __init__(self, eos, NDIFF_REMAPPING_SCHEME="PLM", NEUTRAL_POS_METHOD=3, DELTA_RHO_FORM="mid_pressure", NDIFF_DRHO_TOL=1.e-10,
                 NDIFF_X_TOL=0., NDIFF_MAX_ITER=10, HARD_FAIL_HEFF=True, NDIFF_REF_PRES=-1.0):
        assert NDIFF_REMAPPING_SCHEME in SCHEMES and NEUTRAL_POS_METHOD in (1, 2, 3) and DELTA_RHO_FORM in FORMS
        self.eos, self.scheme, self.neutral_pos_method, self.delta_rho_form = eos, NDIFF_REMAPPING_SCHEME, NEUTRAL_POS_METHOD, DELTA_RHO_FORM
        self.deg = 1 if NDIFF_REMAPPING_SCHEME == "PLM" else 2
        self.drho_tol, self.x_tol, self.max_iter = float(NDIFF_DRHO_TOL), float(NDIFF_X_TOL), int(NDIFF_MAX_ITER)
        self.hard_fail_heff, self.ref_pres = bool(HARD_FAIL_HEFF), float(NDIFF_REF_PRES)
        self.iters = []      # the iterations every search of method 2 or 3 took


def evaluation_polynomial(coeff, ncoef, x):
    """src/ALE/polynomial_functions.F90:19 (x**0 is 1 for every x; x**2 is one product)"""
    f = 0.0
    for k in range(ncoef):
        f = f + coeff[k] * (1.0 if k == 0 else x if k == 1 else x * x)
    return f


def first_derivative_polynomial(coeff, ncoef, x):
    """:46"""
    f = 0.0
    for k in range(1, ncoef):
        f = f + float(k) * coeff[k] * (1.0 if k == 1 else x)
    return f


def build_reconstructions_1d(scheme, deg, h, u, h_neglect, h_neglect_edge):
    """MOM_remapping.F90:257 for PLM, PPM_H4 and PPM_IH4 without boundary extrapolation: (coefficients [n][deg+1], edge values [n][2],
    the integration method)"""
    n = len(u)
    local = scheme
    if n <= 1:
        local = "PCM"
    elif n <= 3:
        local = "PLM"
    elif n <= 4 and scheme == "PPM_IH4":
        local = "PPM_H4"
    if local == "PCM":
        return [[u[k]] + [0.0] * deg for k in range(n)], [[u[k], u[k]] for k in range(n)], 0
    if local == "PLM":
        E, co = orc.plm_reconstruction(h, u, h_neglect)
        method = 1
    else:
        if local == "PPM_H4":
            E0 = orc.edge_values_explicit_h4(h, u, h_neglect_edge)
        else:
            eL, eR = orc.edge_values("ih4", h, u, h_neglect_edge)
            E0 = np.array([eL, eR])
        E, co = orc.ppm_reconstruction(h, u, E0, h_neglect)
        method = 3
    return [[float(co[q, k]) for q in range(deg + 1)] for k in range(n)], [[float(E[0, k]), float(E[1, k])] for k in range(n)], method


def average_value_ppoly(u0, E, coefs, method, i0, xa, xb):
    """MOM_remapping.F90:998 for INTEGRATION_PCM, _PLM and _PPM (i0 0-based)"""
    if xb > xa:
        if method == 0:
            return u0[i0]
        if method == 1:
            return coefs[i0][0] + coefs[i0][1] * 0.5 * (xb + xa)
        mx = 0.5 * (xa + xb)
        a_L, a_R, u_c = E[i0][0], E[i0][1], u0[i0]
        a_c = 0.5 * ((u_c - a_L) + (u_c - a_R))
        if mx < 0.5:
            xa2b2ab = (xa * xa + xb * xb) + xa * xb
            return a_L + ((a_R - a_L) * mx + a_c * (3. * (xb + xa) - 2. * xa2b2ab))
        Ya, Yb = 1. - xa, 1. - xb
        my = 0.5 * (Ya + Yb)
        Ya2b2ab = (Ya * Ya + Yb * Yb) + Ya * Yb
        return a_R + ((a_L - a_R) * my + a_c * (3. * (Yb + Ya) - 2. * Ya2b2ab))
    a_L, a_R = E[i0][0], E[i0][1]
    Ya = 1. - xa
    if method == 0:
        return a_L
    if method == 1:
        if xa < 0.5:
            return a_L + xa * (a_R - a_L)
        return a_R + Ya * (a_L - a_R)
    a_c = 3. * ((u0[i0] - a_L) + (u0[i0] - a_R))
    if xa < 0.5:
        return a_L + xa * ((a_R - a_L) + a_c * Ya)
    return a_R + Ya * ((a_L - a_R) + a_c * xa)


def calc_delta_rho_and_derivs(CS, T1, S1, p1_in, T2, S2, p2_in):
    """:2177: (drho, drdt1, drds1, drdt2, drds2); the derivatives are None where the reference leaves them unset"""
    if CS.ref_pres > 0.:
        p1 = p2 = CS.ref_pres
    else:
        p1, p2 = p1_in, p2_in
    if CS.delta_rho_form == "full":
        pmid = 0.5 * (p1 + p2)
        rho1 = orc.eos_density(CS.eos, T1, S1, pmid)
        rho2 = orc.eos_density(CS.eos, T2, S2, pmid)
        return rho1 - rho2, None, None, None, None
    if CS.delta_rho_form == "mid_pressure":
        pmid = 0.5 * (p1 + p2)
        if CS.ref_pres >= 0:
            pmid = CS.ref_pres
        drdt1, drds1 = orc.eos_density_derivs(CS.eos, T1, S1, pmid)
        drdt2, drds2 = orc.eos_density_derivs(CS.eos, T2, S2, pmid)
    else:
        drdt1, drds1 = orc.eos_density_derivs(CS.eos, T1, S1, p1)
        drdt2, drds2 = orc.eos_density_derivs(CS.eos, T2, S2, p2)
    drho = 0.5 * ((drdt1 + drdt2) * (T1 - T2) + (drds1 + drds2) * (S1 - S2))
    return drho, drdt1, drds1, drdt2, drds2


def mark_unstable_cells(CS, nk, T, S, P):
    """:1841"""
    out = []
    for k in range(nk):
        d = calc_delta_rho_and_derivs(CS, T[k][1], S[k][1], max(P[k][1], CS.ref_pres), T[k][0], S[k][0], max(P[k][0], CS.ref_pres))[0]
        out.append(d > 0.)
    return out


def find_neutral_pos_linear(CS, z0, T_ref, S_ref, dRdT_ref, dRdS_ref, dRdT_top, dRdS_top, dRdT_bot, dRdS_bot, ppoly_T, ppoly_S):
    """:1964"""
    nterm = len(ppoly_T)
    dRdT_diff = dRdT_bot - dRdT_top
    dRdS_diff = dRdS_bot - dRdS_top
    zmin = z0
    zmax = 1.
    a1 = 1. - zmin
    a2 = zmin
    T_z = evaluation_polynomial(ppoly_T, nterm, zmin)
    S_z = evaluation_polynomial(ppoly_S, nterm, zmin)
    dRdT_z = a1 * dRdT_top + a2 * dRdT_bot
    dRdS_z = a1 * dRdS_top + a2 * dRdS_bot
    drho_min = 0.5 * ((dRdT_z + dRdT_ref) * (T_z - T_ref) + (dRdS_z + dRdS_ref) * (S_z - S_ref))
    T_z = evaluation_polynomial(ppoly_T, nterm, 1.)
    S_z = evaluation_polynomial(ppoly_S, nterm, 1.)
    drho_max = 0.5 * ((dRdT_bot + dRdT_ref) * (T_z - T_ref) + (dRdS_bot + dRdS_ref) * (S_z - S_ref))
    if drho_min >= 0.:
        return z0
    elif drho_max == 0.:
        return 1.
    if math.copysign(1., drho_min) == math.copysign(1., drho_max):
        raise RuntimeError("drho_min is the same sign as dhro_max")
    z = z0
    ztest = z0
    n = 0
    for it in range(CS.max_iter):
        n += 1
        a1 = 1. - z
        a2 = z
        dRdT_z = a1 * dRdT_top + a2 * dRdT_bot
        dRdS_z = a1 * dRdS_top + a2 * dRdS_bot
        T_z = evaluation_polynomial(ppoly_T, nterm, z)
        S_z = evaluation_polynomial(ppoly_S, nterm, z)
        drho = 0.5 * ((dRdT_z + dRdT_ref) * (T_z - T_ref) + (dRdS_z + dRdS_ref) * (S_z - S_ref))
        if abs(drho) <= CS.drho_tol:
            break
        if drho < 0. and drho > drho_min:
            drho_min = drho
            zmin = z
        elif drho > 0. and drho < drho_max:
            drho_max = drho
            zmax = z
        dT_dz = first_derivative_polynomial(ppoly_T, nterm, z)
        dS_dz = first_derivative_polynomial(ppoly_S, nterm, z)
        drho_dz = 0.5 * ((dRdT_diff * (T_z - T_ref) + (dRdT_ref + dRdT_z) * dT_dz) + (dRdS_diff * (S_z - S_ref) + (dRdS_ref + dRdS_z) * dS_dz))
        ztest = z - drho / drho_dz if drho_dz != 0. else math.copysign(math.inf, -drho) if drho != 0. else math.nan
        if ztest < zmin or ztest > zmax:
            if drho < 0.:
                ztest = 0.5 * (z + zmax)
            else:
                ztest = 0.5 * (zmin + z)
        if abs(z - ztest) <= CS.x_tol:
            break
        z = ztest
    CS.iters.append(n)
    return z


def find_neutral_pos_full(CS, z0, T_ref, S_ref, P_ref, P_top, P_bot, ppoly_T, ppoly_S):
    """:2084"""
    side = 0
    b = z0
    c = 1.
    nterm = len(ppoly_T)
    Tb = evaluation_polynomial(ppoly_T, nterm, b)
    Sb = evaluation_polynomial(ppoly_S, nterm, b)
    Pb = P_top * (1. - b) + P_bot * b
    drho_b = calc_delta_rho_and_derivs(CS, Tb, Sb, Pb, T_ref, S_ref, P_ref)[0]
    Tc = evaluation_polynomial(ppoly_T, nterm, 1.)
    Sc = evaluation_polynomial(ppoly_S, nterm, 1.)
    Pc = P_bot
    drho_c = calc_delta_rho_and_derivs(CS, Tc, Sc, Pc, T_ref, S_ref, P_ref)[0]
    if drho_b >= 0.:
        return z0
    elif drho_c == 0.:
        return 1.
    if math.copysign(1., drho_b) == math.copysign(1., drho_c):
        return z0
    a = z0
    n = 0
    try:
        for it in range(CS.max_iter):
            n += 1
            a = (drho_b * c - drho_c * b) / (drho_b - drho_c)
            Ta = evaluation_polynomial(ppoly_T, nterm, a)
            Sa = evaluation_polynomial(ppoly_S, nterm, a)
            Pa = P_top * (1. - a) + P_bot * a
            drho_a = calc_delta_rho_and_derivs(CS, Ta, Sa, Pa, T_ref, S_ref, P_ref)[0]
            if abs(drho_a) < CS.drho_tol:
                return a
            if drho_a * drho_c > 0.:
                if abs(a - c) < CS.x_tol:
                    return a
                c = a
                drho_c = drho_a
                if side == -1:
                    drho_b = 0.5 * drho_b
                side = -1
            elif drho_b * drho_a > 0:
                if abs(a - b) < CS.x_tol:
                    return a
                b = a
                drho_b = drho_a
                if side == 1:
                    drho_c = 0.5 * drho_c
                side = 1
            else:
                return a
        return a
    finally:
        CS.iters.append(n)


def search_other_column(CS, ksurf, pos_last, T_from, S_from, P_from, T_top, S_top, P_top, T_bot, S_bot, P_bot, T_poly, S_poly):
    """:1860 (ksurf 1-based)"""
    dRhoTop, dRdT_top, dRdS_top, dRdT_from, dRdS_from = calc_delta_rho_and_derivs(CS, T_top, S_top, P_top, T_from, S_from, P_from)
    dRhoBot, dRdT_bot, dRdS_bot, dRdT_from, dRdS_from = calc_delta_rho_and_derivs(CS, T_bot, S_bot, P_bot, T_from, S_from, P_from)
    if dRhoTop > 0. or ksurf == 1:
        return pos_last
    elif dRhoTop > dRhoBot:
        return 1.
    elif dRhoTop < 0. and dRhoBot < 0.:
        return 1.
    elif dRhoTop == 0. and dRhoBot == 0.:
        return 1.
    elif dRhoBot == 0.:
        return 1.
    elif dRhoTop == 0.:
        return pos_last
    if CS.neutral_pos_method == 1:
        return float(orc.ndiff_ifndp(dRhoTop, P_top, dRhoBot, P_bot))
    if CS.neutral_pos_method == 2:
        return find_neutral_pos_linear(CS, pos_last, T_from, S_from, dRdT_from, dRdS_from, dRdT_top, dRdS_top, dRdT_bot, dRdS_bot, T_poly, S_poly)
    return find_neutral_pos_full(CS, pos_last, T_from, S_from, P_from, P_top, P_bot, T_poly, S_poly)


def find_neutral_surface_positions_discontinuous(CS, nk, Pres_l, hcol_l, Tl, Sl, ppoly_T_l, ppoly_S_l, stable_l, Pres_r, hcol_r, Tr, Sr,
                                                 ppoly_T_r, ppoly_S_r, stable_r, hard_fail_heff=True):
    """:1604 without k_bot / zeta_bot (calc_coeffs passes none).  Layer numbers are the reference's (1-based); the lists are 0-based"""
    ns = 4 * nk
    PoL, PoR, KoL, KoR, hEff = [0.0] * ns, [0.0] * ns, [1] * ns, [1] * ns, [0.0] * (ns - 1)
    ki_right = ki_left = kl_left = kl_right = 1
    lastP_left = lastP_right = 0.
    reached_bottom = False
    s_left = s_right = False      # searching_left_column, searching_right_column

    def increment(kl, ki, this, other):      # increment_interface :1931 -> kl, ki, reached_bottom, searching_this, searching_other
        if ki == 2:
            if kl < nk:
                return kl + 1, 1, False, this, other
            return kl, ki, True, False, True
        return kl, 2, False, this, other

    for k in range(ns):
        ks = k + 1
        if ks == ns:
            PoL[k] = 1.; PoR[k] = 1.; KoL[k] = nk; KoR[k] = nk
        elif not stable_l[kl_left - 1]:
            if ks > 1:
                PoL[k] = float(ki_left - 1); KoL[k] = kl_left; PoR[k] = PoR[k - 1]; KoR[k] = KoR[k - 1]
            else:
                PoR[k] = 0.; KoR[k] = 1; PoL[k] = 0.; KoL[k] = 1
            kl_left, ki_left, reached_bottom, s_left, s_right = increment(kl_left, ki_left, s_left, s_right)
            s_left, s_right = True, False
        elif not stable_r[kl_right - 1]:
            if ks > 1:
                PoR[k] = float(ki_right - 1); KoR[k] = kl_right; PoL[k] = PoL[k - 1]; KoL[k] = KoL[k - 1]
            else:
                PoR[k] = 0.; KoR[k] = 1; PoL[k] = 0.; KoL[k] = 1
            kl_right, ki_right, reached_bottom, s_right, s_left = increment(kl_right, ki_right, s_right, s_left)
            s_left, s_right = False, True
        else:
            dRho = calc_delta_rho_and_derivs(CS, Tr[kl_right - 1][ki_right - 1], Sr[kl_right - 1][ki_right - 1], Pres_r[kl_right - 1][ki_right - 1],
                                             Tl[kl_left - 1][ki_left - 1], Sl[kl_left - 1][ki_left - 1], Pres_l[kl_left - 1][ki_left - 1])[0]
            if not reached_bottom:
                if dRho < 0.:
                    s_left, s_right = True, False
                elif dRho > 0.:
                    s_left, s_right = False, True
                elif kl_left + kl_right == 2 and ki_left + ki_right == 2:
                    s_left, s_right = True, False
                else:
                    s_left, s_right = not s_left, not s_right
            if s_left:
                PoR[k] = ki_right - 1.
                KoR[k] = kl_right
                a = kl_left - 1
                PoL[k] = search_other_column(CS, ks, lastP_left, Tr[kl_right - 1][ki_right - 1], Sr[kl_right - 1][ki_right - 1],
                                             Pres_r[kl_right - 1][ki_right - 1], Tl[a][0], Sl[a][0], Pres_l[a][0], Tl[a][1], Sl[a][1], Pres_l[a][1],
                                             ppoly_T_l[a], ppoly_S_l[a])
                KoL[k] = kl_left
                kl_right, ki_right, reached_bottom, s_right, s_left = increment(kl_right, ki_right, s_right, s_left)
                lastP_left = PoL[k]
                if kl_right == KoR[k] + 1:
                    lastP_right = 0.
            elif s_right:
                PoL[k] = ki_left - 1.
                KoL[k] = kl_left
                a = kl_right - 1
                PoR[k] = search_other_column(CS, ks, lastP_right, Tl[kl_left - 1][ki_left - 1], Sl[kl_left - 1][ki_left - 1],
                                             Pres_l[kl_left - 1][ki_left - 1], Tr[a][0], Sr[a][0], Pres_r[a][0], Tr[a][1], Sr[a][1], Pres_r[a][1],
                                             ppoly_T_r[a], ppoly_S_r[a])
                KoR[k] = kl_right
                kl_left, ki_left, reached_bottom, s_left, s_right = increment(kl_left, ki_left, s_left, s_right)
                lastP_right = PoR[k]
                if kl_left == KoL[k] + 1:
                    lastP_left = 0.
            else:
                raise RuntimeError("Else what?")
        if ks > 1:
            if KoL[k] == KoL[k - 1] and KoR[k] == KoR[k - 1]:
                hL = (PoL[k] - PoL[k - 1]) * hcol_l[KoL[k] - 1]
                hR = (PoR[k] - PoR[k - 1]) * hcol_r[KoR[k] - 1]
                if hL < 0. or hR < 0.:
                    if hard_fail_heff:
                        raise NegativeThickness("Negative thicknesses in neutral diffusion")
                    if s_left:
                        PoL[k] = PoL[k - 1]; KoL[k] = KoL[k - 1]
                    elif s_right:
                        PoR[k] = PoR[k - 1]; KoR[k] = KoR[k - 1]
                elif hL + hR == 0.:
                    hEff[k - 1] = 0.
                else:
                    hEff[k - 1] = 2. * ((hL * hR) / (hL + hR))
            else:
                hEff[k - 1] = 0.
    return PoL, PoR, KoL, KoR, hEff


def neutral_surface_T_eval(nk, k_sub, Ks, Ps, T_mean, T_int, deg, method, T_poly):
    """:2478 (k_sub 0-based): T_top, T_bot, T_sub, T_top_int, T_bot_int"""
    kl = Ks[k_sub] - 1
    pt, pb = Ps[k_sub], Ps[k_sub + 1]
    if pt == 0. and pb == 1.:
        T_top = T_int[kl][0]
        T_bot = T_int[kl][1]
    else:
        if kl > 0 and pt == 0.:
            T_top = T_int[kl - 1][1]
        else:
            T_top = evaluation_polynomial(T_poly[kl], deg + 1, pt)
        if kl < nk - 1 and pb == 1.:
            T_bot = T_int[kl + 1][0]
        else:
            T_bot = evaluation_polynomial(T_poly[kl], deg + 1, pb)
    T_sub = average_value_ppoly(T_mean, T_int, T_poly, method, kl, pt, pb)
    return T_top, T_bot, T_sub, evaluation_polynomial(T_poly[kl], deg + 1, pt), evaluation_polynomial(T_poly[kl], deg + 1, pb)


def neutral_surface_flux(CS, nk, hl, hr, Tl, Tr, PiL, PiR, KoL, KoR, hEff, h_neglect):
    """:2297, the discontinuous branch with khtr_ave = 1"""
    ns = 4 * nk
    cl, Tid_l, ml = build_reconstructions_1d(CS.scheme, CS.deg, hl, Tl, h_neglect, h_neglect)
    cr, Tid_r, mr = build_reconstructions_1d(CS.scheme, CS.deg, hr, Tr, h_neglect, h_neglect)
    Flx = [0.0] * (ns - 1)
    for ks in range(ns - 1):
        if hEff[ks] == 0.:
            continue
        lt, lb, lsub, lti, lbi = neutral_surface_T_eval(nk, ks, KoL, PiL, Tl, Tid_l, CS.deg, ml, cl)
        rt, rb, rsub, rti, rbi = neutral_surface_T_eval(nk, ks, KoR, PiR, Tr, Tid_r, CS.deg, mr, cr)
        dT_top = rt - lt
        dT_bottom = rb - lb
        dT_sublayer = rsub - lsub
        dT_top_int = rti - lti
        dT_bot_int = rbi - lbi
        down = dT_top <= 0. and dT_bottom <= 0. and dT_sublayer <= 0. and dT_top_int <= 0. and dT_bot_int <= 0.
        down = down or (dT_top >= 0. and dT_bottom >= 0. and dT_sublayer >= 0. and dT_top_int >= 0. and dT_bot_int >= 0.)
        if down:
            Flx[ks] = dT_sublayer * hEff[ks] * 1.0
    return Flx


def neutral_diffusion_calc_coeffs(g, h, T, S, CS, ND, p_surf=None, h_ML=None):
    """:337-602 with continuous_reconstruction false.  ND: an ndiff_checker.NDCS (interior_only, H_to_RZ, and where the surfaces go)"""
    nk = g.nk
    hn = g.H_subroundoff
    gH = g.g_Earth * ND.H_to_RZ
    if ND.interior_only:
        if h_ML is None:
            raise RuntimeError("hor_bnd_diffusion requires that visc%h_ML is associated.")
        ND.hbl = np.array(h_ML, dtype=np.float64)
        orc.halo_update(g, ND.hbl, _abi.POS_H)
    cols = {}
    for j in range(g.jsc - 1, g.jec + 2):
        for i in range(g.isc - 1, g.iec + 2):
            c = (j - 1, i - 1)
            hc, Tc, Sc = nc.col(h, c), nc.col(T, c), nc.col(S, c)
            k_bot = 1
            if ND.interior_only and g.mask2dT[c] > 0.:
                _, _, k_bot, _ = boundary_k_range(SURFACE, nk, hc, float(ND.hbl[c]))
            P = [[0.0, 0.0] for _ in range(nk)]
            ps = float(p_surf[c]) if p_surf is not None else None
            if ps is not None:
                P[0][0] = ps
                P[0][1] = ps + hc[0] * gH
            else:
                P[0][0] = 0.
                P[0][1] = hc[0] * gH
            for k in range(1, nk):
                P[k][0] = P[k - 1][1]
                P[k][1] = P[k - 1][1] + hc[k] * gH
            pT, _, _ = build_reconstructions_1d(CS.scheme, CS.deg, hc, Tc, hn, hn)
            pS, _, _ = build_reconstructions_1d(CS.scheme, CS.deg, hc, Sc, hn, hn)
            Ti = [[evaluation_polynomial(pT[k], CS.deg + 1, 0.), evaluation_polynomial(pT[k], CS.deg + 1, 1.)] for k in range(nk)]
            Si = [[evaluation_polynomial(pS[k], CS.deg + 1, 0.), evaluation_polynomial(pS[k], CS.deg + 1, 1.)] for k in range(nk)]
            stable = mark_unstable_cells(CS, nk, Ti, Si, P)
            if ND.interior_only:
                for k in range(k_bot):
                    stable[k] = False
            cols[c] = (P, hc, Ti, Si, pT, pS, stable)
    ND.surf, ND.taper = [], []
    for d, f, cL, cR, wet in nc.faces(g):
        ND.taper.append(None)
        if not wet:
            ND.surf.append(None)
            continue
        ND.surf.append(find_neutral_surface_positions_discontinuous(CS, nk, *cols[cL], *cols[cR], hard_fail_heff=CS.hard_fail_heff))


def neutral_diffusion(g, h, Coef_x, Coef_y, tr, CS, ND, conc_underflow=None):
    """:605-1019 with the fluxes of the discontinuous branch: ndiff_checker.neutral_diffusion's update (:880-914) over 4 nk surfaces a
    face, without the coefficient modes"""
    nk = g.nk
    ns = 4 * nk
    Hs = g.H_subroundoff
    fl = nc.faces(g)
    for m, t in enumerate(tr):
        uFlx, vFlx = {}, {}
        for (d, f, cL, cR, wet), surf in zip(fl, ND.surf):
            F = [0.0] * (ns - 1)
            if wet:
                PoL, PoR, KoL, KoR, hEff = surf
                F = neutral_surface_flux(CS, nk, nc.col(h, cL), nc.col(h, cR), nc.col(t, cL), nc.col(t, cR), PoL, PoR, KoL, KoR, hEff, Hs)
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
                kE, kW = (sE[2] if sE else one), (sW[3] if sW else one)
                kN, kS = (sN[2] if sN else one), (sS[3] if sS else one)
                cE, cW = float(Coef_x[0, j - 1, i]), float(Coef_x[0, j - 1, i - 1])
                cN, cS = float(Coef_y[0, j, i - 1]), float(Coef_y[0, j - 1, i - 1])
                if ND.ndiff_answer_date <= 20240330:
                    dT = [0.0] * nk
                    for ks in range(ns - 1):
                        k = kE[ks] - 1; dT[k] = dT[k] + cE * fE[ks]
                        k = kW[ks] - 1; dT[k] = dT[k] - cW * fW[ks]
                        k = kN[ks] - 1; dT[k] = dT[k] + cN * fN[ks]
                        k = kS[ks] - 1; dT[k] = dT[k] - cS * fS[ks]
                else:
                    dN, dS, dE, dW = [0.0] * nk, [0.0] * nk, [0.0] * nk, [0.0] * nk
                    for ks in range(ns - 1):
                        k = kE[ks] - 1; dE[k] = dE[k] + cE * fE[ks]
                        k = kW[ks] - 1; dW[k] = dW[k] - cW * fW[ks]
                        k = kN[ks] - 1; dN[k] = dN[k] + cN * fN[ks]
                        k = kS[ks] - 1; dS[k] = dS[k] - cS * fS[ks]
                    dT = [(dN[k] + dS[k]) + (dE[k] + dW[k]) for k in range(nk)]
                for k in range(nk):
                    x = float(t[k, j - 1, i - 1]) + dT[k] * (float(g.IareaT[j - 1, i - 1]) / (float(h[k, j - 1, i - 1]) + Hs))
                    if abs(x) < cu:
                        x = 0.0
                    new[(k, j - 1, i - 1)] = x
        for idx, x in new.items():
            t[idx] = x


def tracer_hordiff_neutral(g, h, dt, tr, KhTr, eos, idx_T=0, idx_S=1, max_diff_CFL=-1.0, check_diffusive_CFL=False, conc_underflow=None,
                           p_surf=None, h_ML=None, recalc_neutral_surf=False, NDIFF_ANSWER_DATE=20240101, stats=None, **disc):
    """the neutral branch of tracer_hordiff (:474-534) with NDIFF_CONTINUOUS = False and a constant KHTR; tr is updated in place.
    disc: the parameters of DiscCS.  stats: a dict that receives the shares the tests assert.  Returns (num_itts, halo_updates, max_CFL)"""
    if KhTr <= 0.0 or not tr:
        return 0, 0, 0.0
    CS = DiscCS(eos, **disc)
    ND = nc.NDCS(g, eos, NDIFF_REF_PRES=CS.ref_pres, NDIFF_ANSWER_DATE=NDIFF_ANSWER_DATE, NDIFF_INTERIOR_ONLY=h_ML is not None)
    khdt_x, khdt_y, num_itts, I_numitts, max_CFL = khdt_and_itts(g, dt, KhTr, max_diff_CFL, check_diffusive_CFL)
    halo_updates = 0
    for t in tr:
        orc.halo_update(g, t, _abi.POS_H)
    halo_updates += 1
    neutral_diffusion_calc_coeffs(g, h, tr[idx_T], tr[idx_S], CS, ND, p_surf, h_ML)
    if stats is not None:
        wet = [s for s in ND.surf if s is not None]
        stats["heff_share"] = sum(sum(1 for x in s[4] if x > 0.) for s in wet) / max(1, sum(len(s[4]) for s in wet))
        stats["inside_share"] = sum(sum(1 for p in s[0] + s[1] if 0. < p < 1.) for s in wet) / max(1, sum(2 * len(s[0]) for s in wet))
        stats["max_iter"] = max(CS.iters) if CS.iters else 0
    Coef_x, Coef_y = nc.interface_coefficients(g, khdt_x, khdt_y, I_numitts)
    for itt in range(1, num_itts + 1):
        if itt > 1:
            for t in tr:
                orc.halo_update(g, t, _abi.POS_H)
            halo_updates += 1
            if recalc_neutral_surf:
                neutral_diffusion_calc_coeffs(g, h, tr[idx_T], tr[idx_S], CS, ND, p_surf, h_ML)
        neutral_diffusion(g, h, Coef_x, Coef_y, tr, CS, ND, conc_underflow)
    return num_itts, halo_updates, max_CFL
