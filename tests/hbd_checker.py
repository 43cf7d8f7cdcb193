"""A plain-Python restatement of horizontal boundary diffusion, USE_HORIZONTAL_BOUNDARY_DIFFUSION (src/tracer/MOM_hor_bnd_diffusion.F90,
called by tracer_hordiff at MOM_tracer_hor_diff.F90:408-472), in the reference's order of operations on Python floats (IEEE fp64).
The vertical remapping is orc.remapping_core_h (the HBD control structure keeps force_bounds_in_subcell = .false., as orc does).

The composed expectation of tracer_hordiff with HBD is `tracer_hordiff_hbd` here (num_itts calls of hor_bnd_diffusion) followed by the
unchanged orc.tracer_hordiff: h does not change, so num_itts is the same in both."""
import math

import numpy as np

from mom6_amd import _abi
from oracle import orc

SURFACE, BOTTOM = -1, 1
DBL_EPSILON = 2.0 ** -52
SCHEMES = ("PCM", "PLM", "PPM_H4", "PPM_IH4", "PPM_CW")


def min2(a, b):
    return a if a < b else b


def max2(a, b):
    return a if a > b else b


class HBDCS:
    """hbd_CS (:40-70) as hor_bnd_diffusion_init (:79-158) leaves it; parameters by their reference names and defaults."""

    def __init__(self, H_subroundoff, HBD_LINEAR_TRANSITION=False, APPLY_LIMITER=True, APPLY_LIMITER_REMAP=False, HBD_BOUNDARY_EXTRAP=False,
                 HBD_REMAPPING_SCHEME="PLM"):
        self.H_subroundoff = H_subroundoff
        self.linear, self.limiter, self.limiter_remap = bool(HBD_LINEAR_TRANSITION), bool(APPLY_LIMITER), bool(APPLY_LIMITER_REMAP)
        self.boundary_extrap, self.scheme = bool(HBD_BOUNDARY_EXTRAP), HBD_REMAPPING_SCHEME

    def remap(self, h0, u0, h1):
        """remapping_core_h(CS%remap_CS, n0, h0, u0, n1, h1, u1, H_subroundoff, H_subroundoff)"""
        return [float(x) for x in orc.remapping_core_h(self.scheme, h0, u0, h1, h_neglect=self.H_subroundoff,
                                                        h_neglect_edge=self.H_subroundoff, boundary_extrapolation=self.boundary_extrap)]


def harmonic_mean(h1, h2):
    """:405-414"""
    if h1 + h2 == 0.:
        return 0.
    return 2. * (h1 * h2) / (h1 + h2)


def sort(x):
    """:447-458, the selection sort (the same values in ascending order)"""
    x = list(x)
    n = len(x)
    for i in range(n - 1):
        loc = i
        for j in range(i + 1, n):
            if x[j] < x[loc]:
                loc = j
        x[i], x[loc] = x[loc], x[i]
    return x


def unique(val, val_max=None):
    """:461-500: the distinct values in ascending order, the list cut after the last value <= val_max"""
    if val_max is not None and val_max > max(val):
        raise RuntimeError("Houston, we've had a problem in unique (val_max cannot be > MAXVAL(val))")
    tmp = []
    min_val = min(val) - 1
    max_val = max(val)
    while min_val < max_val:
        min_val = min(v for v in val if v > min_val)
        tmp.append(min_val)
    i = len(tmp)
    if val_max is not None:
        for j in range(len(tmp)):
            if tmp[j] <= val_max:
                i = j + 1
    return tmp[:i]


def merge_interfaces(nk, h_L, h_R, hbl_L, hbl_R, H_subroundoff):
    """:517-573 -> the thicknesses of the HBD grid"""
    n = 2 * nk + 3
    eta_L, eta_R, eta_all = [0.0] * (nk + 1), [0.0] * (nk + 1), [0.0] * n
    kk = 0
    for k in range(1, nk + 1):
        eta_L[k] = eta_L[k - 1] + float(h_L[k - 1])
        eta_R[k] = eta_R[k - 1] + float(h_R[k - 1])
        kk += 2
        eta_all[kk - 1] = eta_L[k]
        eta_all[kk] = eta_R[k]
    eta_all[kk + 1] = float(hbl_L)
    eta_all[kk + 2] = float(hbl_R)
    min_depth = min2(max(eta_L), max(eta_R))
    max_bld = max2(float(hbl_L), float(hbl_R))
    max_depth = min2(min_depth, max_bld)
    eta_unique = unique(sort(eta_all), max_depth)
    return [(eta_unique[k + 1] - eta_unique[k]) + H_subroundoff for k in range(len(eta_unique) - 1)]


def flux_limiter(F_layer, area_L, area_R, phi_L, phi_R, h_L, h_R):
    """:576-605; SIGN(1., x) as the reference build evaluates it (copysign: SIGN(1., -0.) = -1)"""
    F_max = -0.2 * ((area_R * (phi_R * h_R)) - (area_L * (phi_L * h_L)))
    if math.copysign(1., F_layer) == math.copysign(1., F_max):
        if F_max >= 0.:
            return min2(F_layer, F_max)
        return max2(F_layer, F_max)
    return 0.0


def boundary_k_range(boundary, nk, h, hbl):
    """:609-673 -> (k_top, zeta_top, k_bot, zeta_bot), k 1-based"""
    h = [float(x) for x in h[:nk]]
    hsum = 0.
    for x in h:
        hsum = hsum + x
    if boundary == SURFACE:
        k_top, zeta_top, k_bot, zeta_bot, htot = 1, 0., 1, 0., 0.
        if hbl == 0.:
            return k_top, zeta_top, k_bot, zeta_bot
        if hbl >= hsum:
            return k_top, zeta_top, nk, 1.
        for k in range(1, nk + 1):
            htot = htot + h[k - 1]
            if htot >= hbl:
                return k_top, zeta_top, k, 1 - (htot - hbl) / h[k - 1]
        return k_top, zeta_top, k_bot, zeta_bot
    if boundary == BOTTOM:
        k_top, zeta_top, k_bot, zeta_bot, htot = nk, 1., nk, 0., 0.
        if hbl == 0.:
            return k_top, zeta_top, k_bot, zeta_bot
        if hbl >= hsum:
            return 1, 1., k_bot, zeta_bot
        for k in range(nk, 0, -1):
            htot = htot + h[k - 1]
            if htot >= hbl:
                return k, 1 - (htot - hbl) / h[k - 1], k_bot, zeta_bot
        return k_top, zeta_top, k_bot, zeta_bot
    raise RuntimeError("Houston, we've had a problem in boundary_k_range")


def reintegrate_column(nsrc, h_src, uh_src, ndest, h_dest):
    """src/ALE/MOM_remapping.F90:925-993"""
    uh_dest = [0.0] * ndest
    k_src = k_dest = 0
    h_dest_rem = h_src_rem = uh_src_rem = 0.
    src_ran_out = False
    while True:
        if h_src_rem == 0. and k_src < nsrc:
            k_src += 1
            h_src_rem = float(h_src[k_src - 1])
            uh_src_rem = float(uh_src[k_src - 1])
            if h_src_rem == 0.:
                continue
        if h_dest_rem == 0. and k_dest < ndest:
            k_dest += 1
            h_dest_rem = float(h_dest[k_dest - 1])
            uh_dest[k_dest - 1] = 0.
            if h_dest_rem == 0.:
                continue
        if k_src == nsrc and h_src_rem == 0.:
            if src_ran_out:
                break
            src_ran_out = True
            continue
        duh = 0.
        if h_src_rem < h_dest_rem:
            dh = h_src_rem
            if dh > 0.:
                duh = uh_src_rem
            h_src_rem = 0.
            uh_src_rem = 0.
            h_dest_rem = max2(0., h_dest_rem - dh)
        elif h_src_rem > h_dest_rem:
            dh = h_dest_rem
            duh = (dh / h_src_rem) * uh_src_rem
            h_src_rem = max2(0., h_src_rem - dh)
            uh_src_rem = uh_src_rem - duh
            h_dest_rem = 0.
        else:
            duh = uh_src_rem
            h_src_rem = 0.
            uh_src_rem = 0.
            h_dest_rem = 0.
        uh_dest[k_dest - 1] = uh_dest[k_dest - 1] + duh
        if k_dest == ndest and (k_src == nsrc or h_dest_rem == 0.):
            break
    return uh_dest


def fluxes_layer_method(boundary, ke, hbl_L, hbl_R, h_L, h_R, phi_L, phi_R, khtr_u, area_L, area_R, nk, dz_top, CS):
    """:677-828 -> F_layer (ke values)"""
    h_L, h_R, phi_L, phi_R = ([float(x) for x in a[:ke]] for a in (h_L, h_R, phi_L, phi_R))
    khtr_u, dz_top = [float(x) for x in khtr_u[:ke + 1]], [float(x) for x in dz_top[:nk]]
    F_layer = [0.0] * ke
    if hbl_L == 0. or hbl_R == 0.:
        return F_layer
    F_z = [0.0] * nk
    if nk > 0:
        phi_L_z = CS.remap(h_L, phi_L, dz_top)
        phi_R_z = CS.remap(h_R, phi_R, dz_top)
    h_vel = [harmonic_mean(h_L[k], h_R[k]) for k in range(ke)]
    khtr_ul = [khtr_u[k] + 0.5 * (khtr_u[k + 1] - khtr_u[k]) for k in range(ke)]
    if nk > 0:
        khtr_ul_z = CS.remap(h_vel, khtr_ul, dz_top)
    k_bot_L = boundary_k_range(boundary, nk, dz_top, hbl_L)[2]
    k_bot_R = boundary_k_range(boundary, nk, dz_top, hbl_R)[2]
    if boundary == SURFACE:
        k_bot_min, k_bot_max = min(k_bot_L, k_bot_R), max(k_bot_L, k_bot_R)
        for k in range(k_bot_min, 0, -1):
            F = -(dz_top[k - 1] * khtr_ul_z[k - 1]) * (phi_R_z[k - 1] - phi_L_z[k - 1])
            if CS.limiter_remap:
                F = flux_limiter(F, area_L, area_R, phi_L_z[k - 1], phi_R_z[k - 1], dz_top[k - 1], dz_top[k - 1])
            F_z[k - 1] = F
        if CS.linear and (k_bot_max - k_bot_min) > 1:      # the linear decay at the base of hbl
            htot = 0.0
            for k in range(k_bot_min + 1, k_bot_max + 1):
                htot = htot + dz_top[k - 1]
            a = -1.0 / htot
            htot = 0.
            for k in range(k_bot_min + 1, k_bot_max + 1):
                wgt = (a * (htot + (dz_top[k - 1] * 0.5))) + 1.0
                F = -(dz_top[k - 1] * khtr_ul_z[k - 1]) * (phi_R_z[k - 1] - phi_L_z[k - 1]) * wgt
                htot = htot + dz_top[k - 1]
                if CS.limiter_remap:
                    F = flux_limiter(F, area_L, area_R, phi_L_z[k - 1], phi_R_z[k - 1], dz_top[k - 1], dz_top[k - 1])
                F_z[k - 1] = F
    F_layer = reintegrate_column(nk, dz_top, F_z, ke, h_vel)
    htot_max = max2(hbl_L, hbl_R) if CS.linear else min2(hbl_L, hbl_R)
    tmp1 = tmp2 = 0.0
    for k in range(ke):
        if CS.limiter and F_layer[k] != 0.:
            F_layer[k] = flux_limiter(F_layer[k], area_L, area_R, phi_L[k], phi_R[k], h_L[k], h_R[k])
        if max2(tmp1 + (h_L[k] * 0.5), tmp2 + (h_R[k] * 0.5)) > htot_max:
            F_layer[k] = 0.
        tmp1 = tmp1 + h_L[k]
        tmp2 = tmp2 + h_R[k]
    return F_layer


def wet_faces(g):
    """(direction, face index, left cell, right cell) of every wet face hor_bnd_diffusion visits (:232-252), as array indices"""
    faces = []
    for j in range(g.jsc, g.jec + 1):
        for I in range(g.isc - 1, g.iec + 1):
            if g.mask2dCu[j - 1, I] > 0.:
                faces.append((0, (j - 1, I), (j - 1, I - 1), (j - 1, I)))
    for J in range(g.jsc - 1, g.jec + 1):
        for i in range(g.isc, g.iec + 1):
            if g.mask2dCv[J, i - 1] > 0.:
                faces.append((1, (J, i - 1), (J - 1, i - 1), (J, i - 1)))
    return faces


def hor_bnd_diffusion(g, h, Coef_x, Coef_y, tr, hbl, CS, conc_underflow=None, fluxes=None):
    """:166-340 on numpy arrays of a one-tile grid: Coef_x, Coef_y 2-D (the same at every interface, as tracer_hordiff sets them); hbl
    with a valid halo; every tracer of tr updated in place on the compute domain.  fluxes: a list that receives (uFlx, vFlx) per tracer"""
    nk = g.nk
    Hs = CS.H_subroundoff
    col = lambda a, c: [float(x) for x in a[:, c[0], c[1]]]
    faces = wet_faces(g)
    grid = []      # hbd_grid :343
    for d, f, cL, cR in faces:
        dz = merge_interfaces(nk, col(h, cL), col(h, cR), float(hbl[cL]), float(hbl[cR]), Hs)
        if len(dz) > 2 + 2 * nk:
            raise RuntimeError("Houston, we've had a problem in hbd_grid (nk cannot be > CS%hbd_nk)")
        grid.append(dz)
    for m, t in enumerate(tr):
        uFlx, vFlx = np.zeros(g.shape3(_abi.POS_U)), np.zeros(g.shape3(_abi.POS_V))
        for (d, f, cL, cR), dz in zip(faces, grid):
            c = float((Coef_x if d == 0 else Coef_y)[f])
            F = fluxes_layer_method(SURFACE, nk, float(hbl[cL]), float(hbl[cR]), col(h, cL), col(h, cR), col(t, cL), col(t, cR),
                                    [c] * (nk + 1), float(g.areaT[cL]), float(g.areaT[cR]), len(dz), dz, CS)
            (uFlx if d == 0 else vFlx)[:, f[0], f[1]] = F
        if fluxes is not None:
            fluxes.append((uFlx, vFlx))
        cu = 0.0 if conc_underflow is None else float(conc_underflow[m])
        IareaT = g.IareaT
        for k in range(nk):
            for j in range(g.jsc, g.jec + 1):
                for i in range(g.isc, g.iec + 1):
                    x = float(t[k, j - 1, i - 1])
                    if g.mask2dT[j - 1, i - 1] > 0.:
                        x = x + (((float(uFlx[k, j - 1, i - 1]) - float(uFlx[k, j - 1, i]))) +
                                 ((float(vFlx[k, j - 1, i - 1]) - float(vFlx[k, j, i - 1])))) * \
                            float(IareaT[j - 1, i - 1]) / (float(h[k, j - 1, i - 1]) + Hs)
                    if cu > 0.0 and abs(x) < cu:
                        x = 0.0
                    t[k, j - 1, i - 1] = x


def khdt_and_itts(g, dt, KhTr, max_diff_CFL=-1.0, check_diffusive_CFL=False):
    """tracer_hordiff :340-434 with a constant KHTR -> khdt_x, khdt_y (u / v arrays), num_itts, I_numitts, max_CFL"""
    khdt_x, khdt_y = g.zeros2(_abi.POS_U), g.zeros2(_abi.POS_V)
    for j in range(g.jsc, g.jec + 1):
        for I in range(g.isc - 1, g.iec + 1):
            kx = dt * (KhTr * (float(g.dy_Cu[j - 1, I]) * float(g.IdxCu[j - 1, I])))
            if max_diff_CFL > 0.0:
                kx = min2(kx, 0.125 * max_diff_CFL * min2(float(g.areaT[j - 1, I - 1]), float(g.areaT[j - 1, I])))
            khdt_x[j - 1, I] = kx
    for J in range(g.jsc - 1, g.jec + 1):
        for i in range(g.isc, g.iec + 1):
            ky = dt * (KhTr * (float(g.dx_Cv[J, i - 1]) * float(g.IdyCv[J, i - 1])))
            if max_diff_CFL > 0.0:
                ky = min2(ky, 0.125 * max_diff_CFL * min2(float(g.areaT[J - 1, i - 1]), float(g.areaT[J, i - 1])))
            khdt_y[J, i - 1] = ky
    num_itts, max_CFL = 1, 0.0
    if check_diffusive_CFL:
        for j in range(g.jsc, g.jec + 1):
            for i in range(g.isc, g.iec + 1):
                cfl = 2.0 * ((float(khdt_x[j - 1, i - 1]) + float(khdt_x[j - 1, i])) +
                             (float(khdt_y[j - 1, i - 1]) + float(khdt_y[j, i - 1]))) * float(g.IareaT[j - 1, i - 1])
                max_CFL = max2(max_CFL, cfl)
        num_itts = max(1, int(math.ceil(max_CFL - 4.0 * DBL_EPSILON)))
    elif max_diff_CFL > 0.0:
        num_itts = max(1, int(math.ceil(max_diff_CFL - 4.0 * DBL_EPSILON)))
    return khdt_x, khdt_y, num_itts, 1.0 / float(num_itts), max_CFL


def tracer_hordiff_hbd(g, h, dt, tr, KhTr, h_ML, CS, max_diff_CFL=-1.0, check_diffusive_CFL=False, conc_underflow=None):
    """the HBD part of tracer_hordiff (:408-472): num_itts calls of hor_bnd_diffusion, each after a pass of the tracers.  tr is updated in
    place; returns the number of passes"""
    if KhTr <= 0.0 or not tr:
        return 0
    if h_ML is None:
        raise RuntimeError("hor_bnd_diffusion requires that visc%h_ML is associated.")
    khdt_x, khdt_y, num_itts, I_numitts, _ = khdt_and_itts(g, dt, KhTr, max_diff_CFL, check_diffusive_CFL)
    Coef_x, Coef_y = I_numitts * khdt_x, I_numitts * khdt_y
    hbl = np.array(h_ML, dtype=np.float64)
    orc.halo_update(g, hbl, _abi.POS_H)
    for _ in range(num_itts):
        for t in tr:
            orc.halo_update(g, t, _abi.POS_H)
        hor_bnd_diffusion(g, h, Coef_x, Coef_y, tr, hbl, CS, conc_underflow)
    return num_itts
