"""horizontal_viscosity with the production options (biharmonic Smagorinsky with the better bounds and the land mask: the set
the bench and the split RK2 step use), which run in hv_chunk_kernel -- one block per tile and chunk of HV_KCH layers, the metrics of
a point in registers across the chunk.  Library == oracle bit for bit: layer counts around the chunk length, partial tiles on the
eastern and northern edges, land in the frame, staged and resident arrays."""
import numpy as np
import pytest

import exact_synth as xs
from helpers import bits_equal
from oracle import orc

DT = 900.0
HV_KCH = 15                    # hor_visc.hip HV_KCH_DEF
TILE = (60, 12)                # hor_visc.hip: the 64 x 16 frame of hv_chunk_kernel less its halo
OPTS = dict(Ah_vel_scale=0.01, Smagorinsky_Ah=1, Smag_bi_const=0.06)      # bench.HOR_VISC
REF_OPTS = dict(AH_VEL_SCALE=0.01, SMAGORINSKY_AH=True, SMAG_BI_CONST=0.06)


def _parity(ni, nj, nk, land, reentrant_x=True, reentrant_y=False, umax=0.3):
    import torch
    from mom6_amd.hor_visc import hor_visc_init, horizontal_viscosity
    from mom6_amd.tracer_advect import DeviceGrid
    g = xs.make_grid(ni, nj, nk, land_frac=land, reentrant_x=reentrant_x, reentrant_y=reentrant_y)
    d = xs.make_state(g, umax=umax)
    ref = orc.horizontal_viscosity(g, orc.hor_visc_cs(g, DT, **OPTS), d["u"], d["v"], d["h"], DT)
    assert np.abs(ref[0]).max() > 0 and np.abs(ref[1]).max() > 0
    dg = DeviceGrid(g)
    try:
        for resident in (True, False):
            CS = hor_visc_init(dg, DT, device_arrays=resident, BIHARMONIC=True, **REF_OPTS)
            N = (lambda a: a.cpu().numpy()) if resident else (lambda a: a)
            X = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if resident else (lambda a: a.copy())
            du, dv = X(np.zeros_like(d["u"])), X(np.zeros_like(d["v"]))
            horizontal_viscosity(X(d["u"]), X(d["v"]), X(d["h"]), du, dv, None, None, dg, CS)
            dg.sync()
            where = ((ni, nj, nk), land, resident)
            assert bits_equal(N(du), ref[0]), (where, "diffu", np.argwhere(N(du) != ref[0])[:3])
            assert bits_equal(N(dv), ref[1]), (where, "diffv", np.argwhere(N(dv) != ref[1])[:3])
    finally:
        dg.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nk", [1, HV_KCH - 1, HV_KCH, HV_KCH + 1, 75])
def test_layer_counts_around_the_chunk(nk):
    """nk below, at and above the chunk length, and the bench's 75 layers (5 chunks); partial tiles in both directions"""
    _parity(2 * TILE[0] + 7, 2 * TILE[1] + 5, nk, land=0.25)


@pytest.mark.gpu
@pytest.mark.parametrize("ni,nj,nk,land,topo", [
    (TILE[0], TILE[1], 3, 0.2, (True, False)),              # one whole tile
    (TILE[0] + 1, TILE[1] + 1, 4, 0.2, (False, False)),     # one-point tiles on the eastern and northern edges
    (10, 8, 2 * HV_KCH + 1, 0.3, (False, False)),           # one partial tile, three chunks, the last of one layer
    (44, 40, 17, 0.3, (True, True)),
    (3 * TILE[0] + 31, TILE[1] - 3, 6, 0.0, (True, False)),   # no land
    (70, 21, HV_KCH + 2, 0.6, (True, False)),                # mostly land
])
def test_partial_tiles_and_land(ni, nj, nk, land, topo):
    _parity(ni, nj, nk, land, reentrant_x=topo[0], reentrant_y=topo[1])
