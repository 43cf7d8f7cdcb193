"""Times tracer_hordiff with the diagnostics of neutral_diffusion and hor_bnd_diffusion (mix_diag=) off and on, on device arrays on the
benchmark grid (beside tools/perf_ndiff.py, tools/perf_hbd.py and tools/perf_flux_diag.py): a neutral-diffusion call of 4 tracers
(NDIFF_INTERIOR_ONLY, both orders of NDIFF_ANSWER_DATE) and a boundary-diffusion call followed by the along-layer loop.  With
MOM6HIP_LIB_PATH pointing at a build of the parent commit only the `off` lines are printed, and they are the parent's (without mix_diag the
wrappers call the entries the parent has): run the two builds in turn, several times, for the comparison of
profiles/tracer_mix_diagnostics.txt.

    python tools/perf_mix_diag.py [--ni 1440 --nj 1080 --nk 75 --reps 5] [--off-only] [--each] [--cases neutral,hbd]

Prints one line a case: the median and the spread (min .. max) of `reps` timed calls in ms, after one warm-up call; --each adds every array
alone.  The last line is the streaming rate of a device-to-device copy, to hold the added times against."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from mom6_amd import _abi, synth  # noqa: E402
from mom6_amd.pressure_force import EOS_init  # noqa: E402
from mom6_amd.tracer_advect import DeviceGrid  # noqa: E402
from mom6_amd.tracer_hor_diff import tracer_hor_diff_init, tracer_hordiff  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    for n, v in (("ni", 1440), ("nj", 1080), ("nk", 75), ("reps", 5)):
        ap.add_argument("--" + n, type=int, default=v)
    ap.add_argument("--off-only", action="store_true", help="time the calls without diagnostics only")
    ap.add_argument("--each", action="store_true", help="time every array alone too")
    ap.add_argument("--cases", default="neutral,hbd", help="which calls to time: neutral, hbd or both (comma-separated)")
    a = ap.parse_args()
    g = synth.make_grid(a.ni, a.nj, a.nk, seed=20241020, land_frac=0.3)
    d = synth.make_dynamics_state(g, seed=1, device="cuda", umax=0.1, eta_amp=0.2)
    dg = DeviceGrid(g)
    gen = torch.Generator(device="cuda").manual_seed(7)
    visc = dict(h_ML=(10.0 + 290.0 * torch.rand(tuple(d["h"].shape[1:]), device="cuda", dtype=torch.float64, generator=gen)).contiguous())
    h = d["h"].clone()
    start = [d["T"].clone(), d["S"].clone(), torch.rand_like(d["T"]), torch.rand_like(d["T"])]
    trs = [t.clone() for t in start]
    tv = dict(T=trs[0], S=trs[1], eqn_of_state=EOS_init("WRIGHT"))
    from mom6_amd._lib import lib
    has_mix = hasattr(lib(), "mom6hip_tracer_hordiff_mix_diag")

    def zeros(n):
        pos, rank = _abi.MIX_DIAG_KINDS[n]
        return torch.zeros(g.shape2(pos) if rank == 2 else g.shape3(pos), dtype=torch.float64, device="cuda")

    def timed(label, CS, tv_, mix=None):
        ms = []
        for r in range(a.reps + 1):
            for t, s0 in zip(trs, start):
                t.copy_(s0)
            torch.cuda.synchronize()
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            if mix is None:
                tracer_hordiff(h, 3600.0, None, None, visc, dg, CS, trs, tv=tv_)
            else:
                tracer_hordiff(h, 3600.0, None, None, visc, dg, CS, trs, tv=tv_, mix_diag=mix)
            e1.record(); torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms = ms[1:]
        print(f"{label:44s} median {statistics.median(ms):9.3f} ms   ({min(ms):.3f} .. {max(ms):.3f})", flush=True)

    cases = [("neutral 20240101", dict(USE_NEUTRAL_DIFFUSION=True, NDIFF_INTERIOR_ONLY=True, NDIFF_ANSWER_DATE=20240101), tv, _abi.ND_MIX_DIAGS if has_mix else ()),
             ("neutral 20240401", dict(USE_NEUTRAL_DIFFUSION=True, NDIFF_INTERIOR_ONLY=True, NDIFF_ANSWER_DATE=20240401), tv, _abi.ND_MIX_DIAGS if has_mix else ()),
             ("hbd + along-layer", dict(USE_HORIZONTAL_BOUNDARY_DIFFUSION=True), None, _abi.HBD_MIX_DIAGS if has_mix else ())]
    for label, params, tv_, names in [c for c in cases if c[0].split()[0] in a.cases.split(",")]:
        CS = tracer_hor_diff_init(KHTR=50.0, **params)
        timed(label + ", diagnostics off", CS, tv_)
        if not has_mix or a.off_only:
            continue
        for sel in ([(n,) for n in names] if a.each else []) + [names]:
            mix = [{n: zeros(n) for n in sel} for _ in trs]
            timed(label + " + " + ("all of them" if len(sel) > 1 else sel[0]), CS, tv_, mix)
            del mix
    src = torch.empty_like(d["T"]); dst = torch.empty_like(src)
    dst.copy_(src); torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        dst.copy_(src)
    e1.record(); torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 5
    print(f"copy of one h-shaped array of {a.nk} layers: {ms:.3f} ms ({src.numel() * 8 / ms / 1.0e6:.0f} GB/s written)", flush=True)
    dg.close()


if __name__ == "__main__":
    main()
