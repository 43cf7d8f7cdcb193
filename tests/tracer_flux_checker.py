"""A numpy restatement of advect_tracer (src/tracer/MOM_tracer_advect.F90:52-1087) and of the along-layer branch of tracer_hordiff
(src/tracer/MOM_tracer_hor_diff.F90:119-612, constant KHTR) WITH the nine flux diagnostics of tracer_type: ad_x, ad_y, ad2d_x, ad2d_y,
advection_xy and df_x, df_y, df2d_x, df2d_y.  Every expression keeps the reference's parenthesisation; a pass is evaluated for all rows of a
layer at once (the fluxes of a pass read the tracers of before the pass, the reference's T_tmp), the layers in the order k = 1..nz, so the
2-D sums are formed in the reference's order.

One thing the reference leaves open is fixed here: advect_x / advect_y read do_i of the cells is-1 and ie+1 (js-1 and je+1) of their own
range in the test `do_i(i,j) .or. do_i(i+1,j)`, and never set them; here they count as false.  (It matters only where a face carries a
flux although the volume of the cell beside it has dropped to zero.)

Arrays are laid out as mom6_amd.grid.Grid lays them out: (nk, nj, ni) with the last axis i, a(i,j) = a[j - jsd, i - isd] at h points,
u(I,j) = u[j - jsd, I - isd + 1], v(i,J) = v[J - jsd + 1, i - isd]; isd = jsd = 1."""
import math

import numpy as np

from mom6_amd import _abi
from oracle import orc

H, U, V = _abi.POS_H, _abi.POS_U, _abi.POS_V
ADV = _abi.ADV_DIAGS
DIFF = _abi.DIFF_DIAGS
TINY = np.finfo(np.float64).tiny


def min2(a, b): return np.where(a < b, a, b)
def max2(a, b): return np.where(a > b, a, b)
def min3(a, b, c): return min2(min2(a, b), c)
def max3(a, b, c): return max2(max2(a, b), c)


def plm_slope(Tp, Tc, Tm, mask):
    dMx = max3(Tp, Tc, Tm) - Tc
    dMn = Tc - min3(Tp, Tc, Tm)
    return mask * np.copysign(np.abs(min3(0.5 * np.abs(Tp - Tm), 2.0 * dMx, 2.0 * dMn)), Tp - Tm)


def ppm_flux(Tp, Tc, Tm, sm, sc, sp, huynh, mask_prod, hh, CFL):
    if huynh:
        aL = (5. * Tc + (2. * Tm - Tp)) / 6.
        aL = max2(min2(Tc, Tm), aL); aL = min2(max2(Tc, Tm), aL)
        aR = (5. * Tc + (2. * Tp - Tm)) / 6.
        aR = max2(min2(Tc, Tp), aR); aR = min2(max2(Tc, Tp), aR)
    else:
        aL = 0.5 * ((Tm + Tc) + (sm - sc) / 3.)
        aR = 0.5 * ((Tc + Tp) + (sc - sp) / 3.)
    dA = aR - aL; mA = 0.5 * (aR + aL)
    c1 = mask_prod * (Tp - Tc) * (Tc - Tm) <= 0.
    c2 = ~c1 & (dA * (Tc - mA) > (dA * dA) / 6.)
    c3 = ~c1 & ~c2 & (dA * (Tc - mA) < -(dA * dA) / 6.)
    aL2 = np.where(c1, Tc, np.where(c2, 3. * Tc - 2. * aR, aL))
    aR2 = np.where(c1, Tc, np.where(c3, 3. * Tc - 2. * aL, aR))
    aL, aR = aL2, aR2
    a6 = 6. * Tc - 3. * (aR + aL)
    return np.where(hh >= 0.0, hh * (aR - 0.5 * CFL * ((aR - aL) - a6 * (1. - 2. / 3. * CFL))),
                    hh * (aL + 0.5 * CFL * ((aR - aL) + a6 * (1. - 2. / 3. * CFL))))


def face_transport(r, r_m, r_p, h_m, h_p, a_m, a_p, min_h):
    """:485-513 / :868-899 -> (the transport taken, CFL, limited)"""
    none = (r == 0.0) | ((r < 0.0) & (h_p <= TINY)) | ((r > 0.0) & (h_m <= TINY))
    neg = r < 0.0
    hup = h_p - a_p * min_h; hlos = max2(0.0, r_p)
    lim_n = (((hup - hlos) + r) < 0.0) & ((0.5 * hup + r) < 0.0)
    hh_n = np.where(lim_n, min3(-0.5 * hup, -hup + hlos, 0.0), r)
    hup = h_m - a_m * min_h; hlos = max2(0.0, -r_m)
    lim_p = (((hup - hlos) - r) < 0.0) & ((0.5 * hup - r) < 0.0)
    hh_p = np.where(lim_p, max3(0.5 * hup, hup - hlos, 0.0), r)
    hh = np.where(neg, hh_n, hh_p)
    CFL = np.where(neg, -hh / np.where(neg, h_p, 1.0), hh / np.where(neg | none, 1.0, h_m))
    return np.where(none, 0.0, hh), np.where(none, 0.0, CFL), np.where(neg, lim_n, lim_p) & ~none


class Advection:
    """the state of one advect_tracer call; run() is the reference's subroutine"""

    def __init__(self, g, h_end, uhtr, vhtr, dt, cs_dt, scheme, tr, diag=None, conc_underflow=None, x_first=None, max_iter=None,
                 use_huynh_stencil_bug=False):
        self.g, self.tr, self.ntr = g, tr, len(tr)
        self.diag = diag if diag is not None else [None] * len(tr)
        self.cu = conc_underflow
        self.usePPM, self.huynh = scheme != "PLM", scheme == "PPM:H3"
        self.stencil = 3 if (self.usePPM and not use_huynh_stencil_bug) else 2
        self.Idt = 1.0 / dt                                                       # :133
        self.max_iter = 2 * int(math.ceil(dt / cs_dt)) + 1 if max_iter is None else max_iter
        self.x_first = (g.first_direction % 2 == 0) if x_first is None else bool(x_first)
        self.h_end, self.uhtr, self.vhtr = h_end, uhtr, vhtr
        self.log = dict(iterations=0, x_rows_skipped_at_start=0, x_rows_done_after_first=0, y_rows_skipped_at_start=0, y_rows_done_after_first=0)

    def d(self, m, name):
        return (self.diag[m] or {}).get(name)

    def run(self):
        g = self.g
        is_, ie, js, je, nz, st = g.isc, g.iec, g.jsc, g.jec, g.nk, self.stencil
        self.hprev, self.uhr, self.vhr = g.zeros3(H), g.zeros3(U), g.zeros3(V)
        cj, ci = slice(js - 1, je), slice(is_ - 1, ie)
        self.uhr[:, cj, is_ - 1:ie + 1] = self.uhtr[:, cj, is_ - 1:ie + 1]
        self.vhr[:, js - 1:je + 1, ci] = self.vhtr[:, js - 1:je + 1, ci]
        aT = g.areaT[cj, ci]
        hp = max2(0.0, aT * self.h_end[:, cj, ci] + ((self.uhr[:, cj, is_:ie + 1] - self.uhr[:, cj, is_ - 1:ie])
                                                    + (self.vhr[:, js:je + 1, ci] - self.vhr[:, js - 1:je, ci])))
        self.hprev[:, cj, ci] = hp + max2(0.0, 1.0e-13 * hp - aT * self.h_end[:, cj, ci])
        self.uh_neglect, self.vh_neglect = g.zeros2(U), g.zeros2(V)
        self.uh_neglect[:, 1:-1] = g.H_subroundoff * min2(g.areaT[:, :-1], g.areaT[:, 1:])
        self.vh_neglect[1:-1, :] = g.H_subroundoff * min2(g.areaT[:-1, :], g.areaT[1:, :])
        for m in range(self.ntr):                                                 # :190-198
            for n in ADV:
                if self.d(m, n) is not None:
                    self.d(m, n)[...] = 0.0
        self.domore_u = np.zeros((nz, g.njh), dtype=bool)                         # (k, j - jsd)
        self.domore_v = np.zeros((nz, g.njh + 1), dtype=bool)                     # (k, J - jsd + 1)
        domore_k = np.ones(nz, dtype=int)
        isv, iev, jsv, jev = is_, ie, js, je
        itt = 0
        for itt in range(1, self.max_iter + 1):
            if isv > is_ - st:
                for a, pos in ((self.uhr, U), (self.vhr, V), (self.hprev, H)):
                    orc.halo_update(g, a, pos)
                for t in self.tr:
                    orc.halo_update(g, t, H)
                nsten = min(is_ - g.isd, g.ied - ie, js - g.jsd, g.jed - je) // st
                isv, jsv, iev, jev = is_ - nsten * st, js - nsten * st, ie + nsten * st, je + nsten * st
                if nsten > 1 or itt == 1:
                    for k in range(nz):
                        if domore_k[k] > 0:
                            nzu = np.any(self.uhr[k][jsv - 1:jev, isv + st - 1:iev - st + 1] != 0.0, axis=1)
                            self.domore_u[k, jsv - 1:jev] |= nzu
                            nzv = np.any(self.vhr[k][jsv + st - 1:jev - st + 1, isv + st - 1:iev - st] != 0.0, axis=1)
                            self.domore_v[k, jsv + st - 1:jev - st + 1] |= nzv
                            domore_k[k] = int(self.domore_u[k, jsv - 1:jev].any() or self.domore_v[k, jsv + st - 1:jev - st + 1].any())
                    if itt == 1:
                        self.log["x_rows_skipped_at_start"] = int((~self.domore_u[:, js - 1:je]).sum())
                        self.log["y_rows_skipped_at_start"] = int((~self.domore_v[:, js - 1:je + 1]).sum())
            isv += st; iev -= st; jsv += st; jev -= st
            for k in range(nz):                                                   # (the layers are independent: one after the other)
                if domore_k[k] <= 0:
                    continue
                if self.x_first:
                    self.advect(0, k, isv, iev, jsv - st, jev + st)
                    self.advect(1, k, isv, iev, jsv, jev)
                    ju0, ju1 = jsv - st, jev + st
                else:
                    self.advect(1, k, isv - st, iev + st, jsv, jev)
                    self.advect(0, k, isv, iev, jsv, jev)
                    ju0, ju1 = jsv, jev
                domore_k[k] = int(self.domore_u[k, ju0 - 1:ju1].any() or self.domore_v[k, jsv - 1:jev + 1].any())
            if itt == 1:
                self.log["x_rows_done_after_first"] = int((~self.domore_u[:, js - 1:je]).sum()) - self.log["x_rows_skipped_at_start"]
                self.log["y_rows_done_after_first"] = int((~self.domore_v[:, js - 1:je + 1]).sum()) - self.log["y_rows_skipped_at_start"]
            if itt >= self.max_iter:
                break
            if isv > is_ - st and domore_k.sum() == 0:
                break
        self.log["iterations"] = itt
        return self

    def advect(self, d, k, is_, ie, js, je):
        """advect_x (d = 0, :329-701) or advect_y (d = 1, :705-1087) of layer k (0-based) over the reference's range arguments.  The y pass
        is the x pass on transposed views: a `line` runs along the direction of the pass."""
        g = self.g
        T_ = (lambda a: a.T) if d else (lambda a: a)
        if d:
            is_, ie, js, je = js, je, is_, ie                   # n = the index along the pass (is_..ie), c = across it (js..je)
        hp, xr = T_(self.hprev[k]), T_((self.vhr if d else self.uhr)[k])      # [c - 1, n - 1] and faces [c - 1, N]
        areaT, IareaT = T_(g.areaT), T_(g.IareaT)
        fmask, negl = T_(g.mask2dCv if d else g.mask2dCu), T_(self.vh_neglect if d else self.uh_neglect)
        C = slice(js - 1, je)                                   # the lines
        N = np.arange(is_ - 1, ie + 1)                          # the faces of a line
        if d:       # the flag belongs to the row of faces J (:868); all lines share it
            act = np.broadcast_to(self.domore_v[k, N][None, :], (je - js + 1, N.size)).copy()
            self.domore_v[k, N] = False
        else:       # the flag belongs to the line j (:407)
            act = np.broadcast_to(self.domore_u[k, C][:, None], (je - js + 1, N.size)).copy()
            self.domore_u[k, C] = False
        min_h = 0.1 * g.Angstrom_H
        with np.errstate(all="ignore"):
            hh, CFL, lim = face_transport(xr[C][:, N], xr[C][:, N - 1], xr[C][:, N + 1], hp[C][:, N - 1], hp[C][:, N], areaT[C][:, N - 1],
                                          areaT[C][:, N], min_h)
            hh = np.where(act, hh, 0.0); CFL = np.where(act, CFL, 0.0); lim = lim & act
            if d:
                self.domore_v[k, N] = lim.any(axis=0)
            else:
                self.domore_u[k, C] = lim.any(axis=1)
            up = np.where(hh >= 0.0, N[None, :], N[None, :] + 1)      # the upwind cell n_up
            mk = fmask[C]
            take = lambda a, idx: np.take_along_axis(a, idx, axis=1)
            flux = []
            for m in range(self.ntr):
                T = T_(self.tr[m][k])[C]
                sl = np.zeros_like(T)
                sl[:, 1:-1] = plm_slope(T[:, 2:], T[:, 1:-1], T[:, :-2], mk[:, 2:-1] * mk[:, 1:-2])      # cell n: faces n and n - 1
                Tc = take(T, up - 1)
                if self.usePPM:
                    f = ppm_flux(take(T, up), Tc, take(T, up - 2), take(sl, up - 2), take(sl, up - 1), take(sl, up), self.huynh,
                                 take(mk, up) * take(mk, up - 1), hh, CFL)
                else:
                    s = take(sl, up - 1)
                    f = np.where(hh >= 0.0, hh * (Tc + 0.5 * s * (1. - CFL)), hh * (Tc - 0.5 * s * (1. - CFL)))
                flux.append(np.where(act, f, 0.0))
            # the remaining transport: x on the lines that were worked on, y on every face of the range (:632-635, :1021-1024)
            r = xr[C][:, N] - hh
            r = np.where(np.abs(r) < negl[C][:, N], 0.0, r)
            xr[C, is_ - 1:ie + 1] = r if d else np.where(act, r, xr[C][:, N])
            # the cells n = is..ie
            e, w = hh[:, 1:], hh[:, :-1]
            cells = slice(is_ - 1, ie)
            h_old = hp[C, cells]
            any_ = (e != 0.0) | (w != 0.0)
            h_new = h_old - (e - w)
            if d:
                h_new = max2(h_new, 0.0)
            do_i = any_ & (h_new > 0.0)
            hmin = g.H_subroundoff * areaT[C, cells]
            thin = h_new < hmin
            hlst = np.where(do_i & thin, h_old + (hmin - h_new), h_old)
            Ihnew = np.where(thin, 1.0 / hmin, 1.0 / np.where(do_i, h_new, 1.0))
            hp[C, cells] = np.where(any_, h_new, h_old)
            doi_f = np.zeros((je - js + 1, N.size + 1), dtype=bool)      # do_i of the cells is-1 .. ie+1: unset ones count as false
            doi_f[:, 1:-1] = do_i
            fmsk = (doi_f[:, :-1] | doi_f[:, 1:]) & act
            for m in range(self.ntr):
                T = T_(self.tr[m][k])
                fe, fw = flux[m][:, 1:], flux[m][:, :-1]
                T[C, cells] = np.where(do_i, (T[C, cells] * hlst - (fe - fw)) * Ihnew, T[C, cells])
                a3, a2, axy = self.d(m, ADV[d]), self.d(m, ADV[2 + d]), self.d(m, "advection_xy")
                if a3 is not None:
                    v = T_(a3[k]); v[C, is_ - 1:ie + 1] = np.where(fmsk, v[C][:, N] + flux[m] * self.Idt, v[C][:, N])
                if a2 is not None:
                    v = T_(a2); v[C, is_ - 1:ie + 1] = np.where(fmsk, v[C][:, N] + flux[m] * self.Idt, v[C][:, N])
                if axy is not None:
                    v = T_(axy[k]); v[C, cells] = np.where(do_i, v[C, cells] - (fe - fw) * self.Idt * IareaT[C, cells], v[C, cells])
                if self.cu is not None and self.cu[m] > 0.0:
                    T[C, cells] = np.where(np.abs(T[C, cells]) < self.cu[m], 0.0, T[C, cells])


def advect_tracer(g, h_end, uhtr, vhtr, dt, cs_dt, scheme, tr, diag=None, **kw):
    """advect_tracer on numpy arrays: the tracers are updated in place, the arrays of diag (an entry a tracer: None or a dict of any of
    ad_x, ad_y, ad2d_x, ad2d_y, advection_xy) are zeroed and filled.  Returns the Advection (its log counts what the inputs exercise)."""
    return Advection(g, h_end, uhtr, vhtr, dt, cs_dt, scheme, tr, diag, **kw).run()


def tracer_hordiff(g, h, dt, tr, KhTr, max_diff_CFL=-1.0, check_diffusive_CFL=False, conc_underflow=None, diag=None, Diffuse_ML_interior=None):
    """the along-layer branch of tracer_hordiff with a constant KHTR (:340-351, :368-398, :410-434, :389-406, :539-607).
    Diffuse_ML_interior: None, or (nkml, nk_rho_varies, ML_KhTr_scale) -- the layers :544-550 scale or leave out; the epipycnal diffusion that
    follows in the reference (:613-620) is NOT restated, so with it only df_x and df_y are the reference's.  Returns num_itts."""
    is_, ie, js, je, nz = g.isc, g.iec, g.jsc, g.jec, g.nk
    ntr = len(tr)
    if ntr == 0 or KhTr <= 0.0:
        return 0
    diag = diag if diag is not None else [None] * ntr
    Idt = 1.0 / dt
    h_neglect = g.H_subroundoff
    cj, ci = slice(js - 1, je), slice(is_ - 1, ie)
    # khdt_x(I,j) I = is-1..ie, j = js..je; khdt_y(i,J) J = js-1..je
    uI = slice(is_ - 1, ie + 1); vJ = slice(js - 1, je + 1)
    kx = dt * (KhTr * (g.dy_Cu[cj, uI] * g.IdxCu[cj, uI]))
    ky = dt * (KhTr * (g.dx_Cv[vJ, ci] * g.IdyCv[vJ, ci]))
    if max_diff_CFL > 0.0:
        kx = min2(kx, 0.125 * max_diff_CFL * min2(g.areaT[cj, is_ - 2:ie], g.areaT[cj, is_ - 1:ie + 1]))
        ky = min2(ky, 0.125 * max_diff_CFL * min2(g.areaT[js - 2:je, ci], g.areaT[js - 1:je + 1, ci]))
    num_itts = 1
    if check_diffusive_CFL:
        cfl = 2.0 * ((kx[:, :-1] + kx[:, 1:]) + (ky[:-1, :] + ky[1:, :])) * g.IareaT[cj, ci]
        num_itts = max(1, int(math.ceil(float(cfl.max()) - 4.0 * np.finfo(float).eps)))
    elif max_diff_CFL > 0.0:
        num_itts = max(1, int(math.ceil(max_diff_CFL - 4.0 * np.finfo(float).eps)))
    I_numitts = 1.0 / float(num_itts)
    for m in range(ntr):                                                          # :389-406
        dd = diag[m] or {}
        if dd.get("df_x") is not None: dd["df_x"][:, cj, uI] = 0.0
        if dd.get("df_y") is not None: dd["df_y"][:, vJ, ci] = 0.0
        if dd.get("df2d_x") is not None: dd["df2d_x"][cj, uI] = 0.0
        if dd.get("df2d_y") is not None: dd["df2d_y"][vJ, ci] = 0.0
    for itt in range(num_itts):
        for t in tr:
            orc.halo_update(g, t, H)
        for k in range(nz):
            scale = I_numitts
            if Diffuse_ML_interior is not None:
                nkml, nkmb, ML_scale = Diffuse_ML_interior
                if k + 1 <= nkml:
                    if ML_scale <= 0.0:
                        continue
                    scale = I_numitts * ML_scale
                if nkml < k + 1 <= nkmb:
                    continue
            hk = h[k]
            Cy = ((scale * ky) * 2.0 * (hk[js - 2:je, ci] * hk[js - 1:je + 1, ci])) / (hk[js - 2:je, ci] + hk[js - 1:je + 1, ci] + h_neglect)
            Cx = ((scale * kx) * 2.0 * (hk[cj, is_ - 2:ie] * hk[cj, is_ - 1:ie + 1])) / (hk[cj, is_ - 2:ie] + hk[cj, is_ - 1:ie + 1] + h_neglect)
            Ihdxdy = g.IareaT[cj, ci] / (hk[cj, ci] + h_neglect)
            for m in range(ntr):
                t = tr[m][k]
                dx = t[cj, is_ - 2:ie] - t[cj, is_ - 1:ie + 1]                    # t(i) - t(i+1) at I = is-1..ie
                dy = t[js - 2:je, ci] - t[js - 1:je + 1, ci]
                dTr = Ihdxdy * ((Cx[:, :-1] * dx[:, :-1] - Cx[:, 1:] * dx[:, 1:]) + (Cy[:-1, :] * dy[:-1, :] - Cy[1:, :] * dy[1:, :]))
                dd = diag[m] or {}
                if dd.get("df_x") is not None: dd["df_x"][k][cj, uI] = dd["df_x"][k][cj, uI] + Cx * dx * Idt
                if dd.get("df_y") is not None: dd["df_y"][k][vJ, ci] = dd["df_y"][k][vJ, ci] + Cy * dy * Idt
                if dd.get("df2d_x") is not None: dd["df2d_x"][cj, uI] = dd["df2d_x"][cj, uI] + Cx * dx * Idt
                if dd.get("df2d_y") is not None: dd["df2d_y"][vJ, ci] = dd["df2d_y"][vJ, ci] + Cy * dy * Idt
                t[cj, ci] = t[cj, ci] + dTr
        if conc_underflow is not None:
            for m in range(ntr):
                if conc_underflow[m] > 0.0:
                    t = tr[m]
                    t[:, cj, ci] = np.where(np.abs(t[:, cj, ci]) < conc_underflow[m], 0.0, t[:, cj, ci])
    return num_itts
