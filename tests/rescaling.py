"""The thickness unit as a run-time choice (the reference's H_RESCALE_POWER, src/core/MOM_verticalGrid.F90:156-175, and its `test.dim.h`).

rescale_grid(g, c) is the grid g with thicknesses held in units of 2^-c of g's thickness unit, so that every thickness is a number 2^c
times as large.  With the Boussinesq branch of verticalGridInit and GV%m_to_H -> 2^c GV%m_to_H:

  GV%Z_to_H         = US%Z_to_m * GV%m_to_H                      x 2^c    (MOM_verticalGrid.F90:199)
  GV%H_to_Z         = GV%H_to_m * US%m_to_Z                      / 2^c    (:198)
  GV%Angstrom_H     = (US%Z_to_m * GV%m_to_H) * GV%Angstrom_Z    x 2^c    (:212)
  GV%H_subroundoff  = 1e-20 * max(GV%Angstrom_H, GV%m_to_H*1e-17) x 2^c   (:215)
  GV%dZ_subroundoff = 1e-20 * max(GV%Angstrom_Z, US%m_to_Z*1e-17) as it was (:216)
  GV%H_to_RZ        = GV%H_to_kg_m2 * ...  = Rho0 * H_to_Z       / 2^c    (:192, :220; the library forms it from the grid)
  GV%RZ_to_H        = GV%kg_m2_to_H * ...  = Z_to_H / Rho0       x 2^c    (:193, :221)

g_Earth, Rho0, every metric, the masks, the topology, first_direction and the halo do not hold a thickness."""
import numpy as np

from mom6_amd.grid import Grid


def rescale_grid(g, c):
    H = 2.0 ** c
    r = Grid(ni=g.ni, nj=g.nj, nk=g.nk, halo=g.halo, reentrant_x=g.reentrant_x, reentrant_y=g.reentrant_y, tripolar_n=g.tripolar_n,
             first_direction=g.first_direction, Angstrom_H=g.Angstrom_H * H, H_to_Z=g.H_to_Z / H, Z_to_H=g.Z_to_H * H, g_Earth=g.g_Earth, Rho0=g.Rho0)
    # the constructor forms the two roundoff thicknesses for any Z_to_H: nothing is overwritten here
    assert r.H_subroundoff == g.H_subroundoff * H and r.dZ_subroundoff == g.dZ_subroundoff, (r.H_subroundoff, g.H_subroundoff)
    assert r.Angstrom_H * r.H_to_Z == g.Angstrom_H * g.H_to_Z and r.H_to_Z * r.Z_to_H == g.H_to_Z * g.Z_to_H
    for n, m in g.metrics.items():
        r.set_metric(n, m)
    return r


def scale_fields(d, exps, c):
    """the named fields of d times 2^(c e), e = exps[name] the power of the thickness unit in the field's units; a list is scaled member by
    member, None is kept, and a name that exps lacks is an error: a field without a stated dimension is not compared"""
    out = {}
    for k, x in d.items():
        e = exps[k]
        if x is None or e is None:      # (e None: not a quantity with units, a record or a count that is kept as it is)
            out[k] = x
        elif isinstance(x, (list, tuple)):
            out[k] = type(x)(scale_fields({k: t}, exps, c)[k] for t in x) if e else x
        else:
            out[k] = x * 2.0 ** (c * e) if e else x
    return out
