"""Times advect_tracer and the along-layer tracer_hordiff with the tracer flux diagnostics off and with each of them on, on device arrays
(beside tools/perf_lateral.py).  With MOM6HIP_LIB_PATH pointing at a build of the parent commit only the `off` lines are printed, and they
are the parent's (without diagnostics the wrappers call the entries the parent has): run the two builds in turn, several times, for the
comparison of profiles/tracer_flux_diagnostics.txt.

    python tools/perf_flux_diag.py [--ni 1440 --nj 1080 --nk 75 --ntr 2 --reps 5]

Prints one line a case: the median and the spread (min .. max) of `reps` timed calls in ms, after one warm-up call."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from mom6_amd import _abi, synth  # noqa: E402
from mom6_amd.tracer_advect import DeviceGrid, advect_tracer, tracer_advect_init  # noqa: E402
from mom6_amd.tracer_hor_diff import tracer_hor_diff_init, tracer_hordiff  # noqa: E402

POS = dict(ad_x=_abi.POS_U, ad_y=_abi.POS_V, ad2d_x=_abi.POS_U, ad2d_y=_abi.POS_V, advection_xy=_abi.POS_H, df_x=_abi.POS_U, df_y=_abi.POS_V,
           df2d_x=_abi.POS_U, df2d_y=_abi.POS_V)


def main():
    ap = argparse.ArgumentParser()
    for n, v in (("ni", 1440), ("nj", 1080), ("nk", 75), ("ntr", 2), ("reps", 5)):
        ap.add_argument("--" + n, type=int, default=v)
    ap.add_argument("--off-only", action="store_true", help="time the calls without diagnostics only")
    a = ap.parse_args()
    g = synth.make_grid(a.ni, a.nj, a.nk, seed=1)
    st = synth.make_advection_state(g, ntr=a.ntr, seed=2, device="cuda")
    dg = DeviceGrid(g, device=0)
    from mom6_amd._lib import lib
    has_diag = hasattr(lib(), "mom6hip_advect_tracer_diag")
    zeros = lambda n: torch.zeros(g.shape2(POS[n]) if "2d" in n else g.shape3(POS[n]), dtype=torch.float64, device="cuda")

    def timed(label, call):
        ms = []
        for r in range(a.reps + 1):
            tr = [t.clone() for t in st["tr"]]
            torch.cuda.synchronize(); t0 = time.perf_counter()
            call(tr)
            dg.sync(); torch.cuda.synchronize()
            ms.append(1.0e3 * (time.perf_counter() - t0))
        ms = ms[1:]
        print(f"{label:34s} median {statistics.median(ms):9.3f} ms   ({min(ms):.3f} .. {max(ms):.3f})", flush=True)

    CSa = tracer_advect_init(900.0, "PPM:H3")
    CSd = tracer_hor_diff_init(KHTR=1000.0, MAX_TR_DIFFUSION_CFL=2.0)
    h = st["h_end"].clone(); dg.halo_update([h], [_abi.POS_H])
    adv = lambda tr, **kw: advect_tracer(st["h_end"], st["uhtr"], st["vhtr"], None, 3600.0, dg, CSa, tr, **kw)
    dif = lambda tr, **kw: tracer_hordiff(h, 3600.0, None, None, None, dg, CSd, tr, **kw)
    timed("advect_tracer, diagnostics off", adv)
    timed("tracer_hordiff, diagnostics off", dif)
    if has_diag and not a.off_only:
        for names in [(n,) for n in _abi.ADV_DIAGS] + [_abi.ADV_DIAGS]:
            d = [{n: zeros(n) for n in names} for m in range(a.ntr)]
            timed("advect_tracer + " + ("all five" if len(names) > 1 else names[0]), lambda tr, d=d: adv(tr, diag=d))
        for names in [(n,) for n in _abi.DIFF_DIAGS] + [_abi.DIFF_DIAGS]:
            d = [{n: zeros(n) for n in names} for m in range(a.ntr)]
            timed("tracer_hordiff + " + ("all four" if len(names) > 1 else names[0]), lambda tr, d=d: dif(tr, diag=d))
    dg.close()


if __name__ == "__main__":
    main()
