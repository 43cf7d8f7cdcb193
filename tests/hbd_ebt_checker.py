"""Horizontal boundary diffusion with KHTR_USE_EBT_STRUCT (src/tracer/MOM_tracer_hor_diff.F90:408-472), by composition: the column
routines are those of hbd_checker (fluxes_layer_method takes khtr_u at every interface already); what changes is the driver, which hands it
the interface coefficients of a face (ndiff_checker.interface_coefficients, with the floor of FULL_DEPTH_KHTR_MIN) where hbd_checker hands
it one constant."""
import numpy as np

from hbd_checker import SURFACE, fluxes_layer_method, khdt_and_itts, max2, merge_interfaces, wet_faces
from mom6_amd import _abi
from ndiff_checker import col, interface_coefficients
from oracle import orc


def hor_bnd_diffusion(g, h, Coef_x, Coef_y, tr, hbl, CS, conc_underflow=None):
    """hbd_checker.hor_bnd_diffusion (:166-340) with Coef_x, Coef_y at the nk+1 interfaces"""
    nk = g.nk
    Hs = CS.H_subroundoff
    faces = wet_faces(g)
    grid = []
    for d, f, cL, cR in faces:
        dz = merge_interfaces(nk, col(h, cL), col(h, cR), float(hbl[cL]), float(hbl[cR]), Hs)
        if len(dz) > 2 + 2 * nk:
            raise RuntimeError("Houston, we've had a problem in hbd_grid (nk cannot be > CS%hbd_nk)")
        grid.append(dz)
    for m, t in enumerate(tr):
        uFlx, vFlx = np.zeros(g.shape3(_abi.POS_U)), np.zeros(g.shape3(_abi.POS_V))
        for (d, f, cL, cR), dz in zip(faces, grid):
            khtr_u = [float(x) for x in (Coef_x if d == 0 else Coef_y)[:, f[0], f[1]]]
            F = fluxes_layer_method(SURFACE, nk, float(hbl[cL]), float(hbl[cR]), col(h, cL), col(h, cR), col(t, cL), col(t, cR),
                                    khtr_u, float(g.areaT[cL]), float(g.areaT[cR]), len(dz), dz, CS)
            (uFlx if d == 0 else vFlx)[:, f[0], f[1]] = F
        cu = 0.0 if conc_underflow is None else float(conc_underflow[m])
        for k in range(nk):
            for j in range(g.jsc, g.jec + 1):
                for i in range(g.isc, g.iec + 1):
                    x = float(t[k, j - 1, i - 1])
                    if g.mask2dT[j - 1, i - 1] > 0.:
                        x = x + (((float(uFlx[k, j - 1, i - 1]) - float(uFlx[k, j - 1, i]))) +
                                 ((float(vFlx[k, j - 1, i - 1]) - float(vFlx[k, j, i - 1])))) * \
                            float(g.IareaT[j - 1, i - 1]) / (float(h[k, j - 1, i - 1]) + Hs)
                    if cu > 0.0 and abs(x) < cu:
                        x = 0.0
                    t[k, j - 1, i - 1] = x


def tracer_hordiff_hbd(g, h, dt, tr, KhTr, h_ML, CS, ebt_struct, KhTr_min=0.0, FULL_DEPTH_KHTR_MIN=False, max_diff_CFL=-1.0,
                       check_diffusive_CFL=False, conc_underflow=None):
    """the HBD part of tracer_hordiff (:408-472) with KHTR_USE_EBT_STRUCT; VarMix%use_variable_mixing is set with it, so the diffusivity
    of a face is max(KHTR, KHTR_MIN) (:238-245).  FULL_DEPTH_KHTR_MIN is read with KHTR_MIN > 0 only (:1667).  Returns the passes"""
    khdt_x, khdt_y, num_itts, I_numitts, _ = khdt_and_itts(g, dt, max2(KhTr, KhTr_min), max_diff_CFL, check_diffusive_CFL)
    floor = KhTr_min if (FULL_DEPTH_KHTR_MIN and KhTr_min > 0.0) else None
    Coef_x, Coef_y = interface_coefficients(g, khdt_x, khdt_y, I_numitts, ebt_struct, floor)
    hbl = np.array(h_ML, dtype=np.float64)
    orc.halo_update(g, hbl, _abi.POS_H)
    for _ in range(num_itts):
        for t in tr:
            orc.halo_update(g, t, _abi.POS_H)
        hor_bnd_diffusion(g, h, Coef_x, Coef_y, tr, hbl, CS, conc_underflow)
    return num_itts
