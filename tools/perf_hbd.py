"""Times tracer_hordiff with and without USE_HORIZONTAL_BOUNDARY_DIFFUSION (KHTR = 50, 4 tracers, visc%h_ML between 10 and 300 m) on the
benchmark grid, device-resident, and prints one JSON line: the times, the difference (the cost of HBD), and the algorithmic bytes of the
HBD kernels.  Run it once plainly and once under `rocprofv3 --kernel-trace --stats -- python tools/perf_hbd.py` for the split by kernel.
Usage: python tools/perf_hbd.py [NIxNJxNK] [SCHEME]"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch

from mom6_amd import synth
from mom6_amd.tracer_advect import DeviceGrid
from mom6_amd.tracer_hor_diff import tracer_hor_diff_init, tracer_hordiff

NI, NJ, NK = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "1440x1080x75").split('x')]
SCHEME = sys.argv[2] if len(sys.argv) > 2 else "PLM"
g = synth.make_grid(NI, NJ, NK, seed=20241020, land_frac=0.3)
d = synth.make_dynamics_state(g, seed=1, device="cuda", umax=0.1, eta_amp=0.2)
dg = DeviceGrid(g)
sh2 = tuple(d["h"].shape[1:])
gen = torch.Generator(device="cuda").manual_seed(7)
h_ML = (10.0 + 290.0 * torch.rand(sh2, device="cuda", dtype=torch.float64, generator=gen)).contiguous()
visc = dict(h_ML=h_ML)
hh = d["h"].clone()
trs = [d["T"].clone(), d["S"].clone(), torch.rand_like(d["T"]), torch.rand_like(d["T"])]


def T(f, n=3):
    f(); torch.cuda.synchronize()
    a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        f()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n


plain = tracer_hor_diff_init(KHTR=50.0)
hbd = tracer_hor_diff_init(KHTR=50.0, USE_HORIZONTAL_BOUNDARY_DIFFUSION=True, HBD_REMAPPING_SCHEME=SCHEME)
t0 = T(lambda: tracer_hordiff(hh, 3600.0, None, None, None, dg, plain, trs))
t1 = T(lambda: tracer_hordiff(hh, 3600.0, None, None, visc, dg, hbd, trs))
cells = NI * NJ
nz_hbd = float((torch.cumsum(hh, 0) - 0.5 * hh <= h_ML[None]).sum(0).double().mean())      # mean layers above hbl per column
mask = float(g.mask2dT.sum()) / ((NI + 2 * g.halo) * (NJ + 2 * g.halo))
print(json.dumps({
    "grid": f"{NI}x{NJ}x{NK}", "ntr": len(trs), "scheme": SCHEME,
    "tracer_hordiff_4tr_ms": t0, "tracer_hordiff_hbd_4tr_ms": t1, "hbd_ms": t1 - t0, "hbd_ms_per_tracer": (t1 - t0) / len(trs),
    "algorithmic_bytes_per_tracer": {
        "hbd_update_kernel": 8 * cells * NK * 3,      # read h and t, write t (fluxes of the few top layers not counted)
        "hbd_flux_kernel_x2": int(2 * cells * mask * NK * 8 * 4),      # h and t of both whole columns of every wet face, two directions
    },
    "mean_layers_above_hbl": nz_hbd}))
