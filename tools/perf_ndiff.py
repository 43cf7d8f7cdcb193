"""Times the neutral branch of tracer_hordiff (USE_NEUTRAL_DIFFUSION, KHTR = 50, 4 tracers) on the benchmark grid, device-resident, with
NDIFF_TAPERING and KHTR_USE_EBT_STRUCT off and on, and prints one JSON line: per mode the median, the smallest and the largest of REPS
measurements (each the mean of N calls after a warm-up call), in ms per call.  The modes: plain (no NDIFF_INTERIOR_ONLY), interior
(NDIFF_INTERIOR_ONLY, both switches off), taper, ebt (with NDIFF_INTERIOR_ONLY), both; and, asked for by name, the discontinuous
reconstructions (NDIFF_CONTINUOUS = False): disc_plm_m3 (PLM, NEUTRAL_POS_METHOD 3, the defaults) and disc_ppm_h4_m1 (PPM_H4, method 1).
A discontinuous mode that stops on a negative sublayer (HARD_FAIL_HEFF) is timed with HARD_FAIL_HEFF = False and says so.  To compare two builds of the library in one
session, run it once with MOM6HIP_LIB_PATH at each; a build without the two modes is given the modes it has.
Usage: python tools/perf_ndiff.py [NIxNJxNK] [REPS] [mode,mode,...]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch

from mom6_amd import synth
from mom6_amd.pressure_force import EOS_init
from mom6_amd.tracer_advect import DeviceGrid
from mom6_amd.tracer_hor_diff import tracer_hor_diff_init, tracer_hordiff

NI, NJ, NK = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "1440x1080x75").split('x')]
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
MODES = (sys.argv[3] if len(sys.argv) > 3 else "plain,interior,taper,ebt,both").split(',')
N = 3
g = synth.make_grid(NI, NJ, NK, seed=20241020, land_frac=0.3)
d = synth.make_dynamics_state(g, seed=1, device="cuda", umax=0.1, eta_amp=0.2)
dg = DeviceGrid(g)
sh2 = tuple(d["h"].shape[1:])
gen = torch.Generator(device="cuda").manual_seed(7)
visc = dict(h_ML=(10.0 + 290.0 * torch.rand(sh2, device="cuda", dtype=torch.float64, generator=gen)).contiguous())
hh = d["h"].clone()
trs = [d["T"].clone(), d["S"].clone(), torch.rand_like(d["T"]), torch.rand_like(d["T"])]
tv = dict(T=trs[0], S=trs[1], eqn_of_state=EOS_init("WRIGHT"))
z = (torch.arange(NK, device="cuda", dtype=torch.float64) / NK)[:, None, None]
VarMix = dict(ebt_struct=torch.clamp(torch.exp(-1.5 * z) + 0.1 * torch.randn(d["h"].shape, device="cuda", dtype=torch.float64, generator=gen),
                                     0.0, 1.0).contiguous())
PARAMS = dict(plain=dict(), interior=dict(NDIFF_INTERIOR_ONLY=True), taper=dict(NDIFF_INTERIOR_ONLY=True, NDIFF_TAPERING=True),
              ebt=dict(NDIFF_INTERIOR_ONLY=True, KHTR_USE_EBT_STRUCT=True),
              both=dict(NDIFF_INTERIOR_ONLY=True, NDIFF_TAPERING=True, KHTR_USE_EBT_STRUCT=True),
              disc_plm_m3=dict(NDIFF_CONTINUOUS=False, NDIFF_REMAPPING_SCHEME="PLM", NEUTRAL_POS_METHOD=3),
              disc_ppm_h4_m1=dict(NDIFF_CONTINUOUS=False, NDIFF_REMAPPING_SCHEME="PPM_H4", NEUTRAL_POS_METHOD=1))


def T(f):
    f(); torch.cuda.synchronize()
    a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(N):
        f()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / N


saved = [t.clone() for t in trs]


def T_restored(f):
    """as T, but every call starts from the first state (restored outside the timed window): the discontinuous search stops on a
    negative sublayer (HARD_FAIL_HEFF), which the state after a few calls of this strength can produce"""
    total = 0.0
    for n in range(N + 1):
        for t, s0 in zip(trs, saved):
            t.copy_(s0)
        torch.cuda.synchronize()
        a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
        a.record(); f(); b.record(); torch.cuda.synchronize()
        if n > 0:      # (the first call is the warm-up)
            total += a.elapsed_time(b)
    return total / N


out = {"grid": f"{NI}x{NJ}x{NK}", "ntr": len(trs), "reps": REPS, "calls_per_rep": N, "ms_per_call": {}}
for mode in MODES:
    CS = tracer_hor_diff_init(KHTR=50.0, USE_NEUTRAL_DIFFUSION=True, **PARAMS[mode])
    soft = False
    if mode.startswith("disc"):
        try:
            tracer_hordiff(hh, 3600.0, None, None, None, dg, CS, trs, tv=tv)
        except Exception as e:
            if "Negative thicknesses" not in str(e):
                raise
            soft = True
            for t, s0 in zip(trs, saved):
                t.copy_(s0)
            CS = tracer_hor_diff_init(KHTR=50.0, USE_NEUTRAL_DIFFUSION=True, HARD_FAIL_HEFF=False, **PARAMS[mode])
    vm = VarMix if PARAMS[mode].get("KHTR_USE_EBT_STRUCT") else None
    vs = visc if PARAMS[mode].get("NDIFF_INTERIOR_ONLY") else None
    ts = [(T_restored if mode.startswith("disc") else T)(lambda: tracer_hordiff(hh, 3600.0, None, vm, vs, dg, CS, trs, tv=tv)) for _ in range(REPS)]
    out["ms_per_call"][mode] = {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}
    if mode.startswith("disc"):
        out["ms_per_call"][mode]["HARD_FAIL_HEFF"] = not soft
        out["ms_per_call"][mode]["device_GB_in_use_after"] = (torch.cuda.mem_get_info()[1] - torch.cuda.mem_get_info()[0]) / 1e9
print(json.dumps(out))
