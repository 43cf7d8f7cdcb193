"""Worker of the two-tile test of horizontal boundary diffusion (tests/test_hor_bnd_diffusion.py); importable by spawned processes."""
import os

from mp_workers import _init


def hbd_layout_worker(rank, world, port, layout, out_dir, neutral=False):
    """test.layout for tracer_hordiff with USE_HORIZONTAL_BOUNDARY_DIFFUSION (several iterations), along layers or with interior-only
    neutral diffusion: the tiles must reproduce the one-tile run bit for bit."""
    import numpy as np
    from mom6_amd import _abi, synth
    from mom6_amd.domains import Domain
    from mom6_amd.pressure_force import EOS_init
    from mom6_amd.tracer_advect import DeviceGrid
    from mom6_amd.tracer_hor_diff import tracer_hor_diff_init, tracer_hordiff
    dist = _init(rank, world, port)
    try:
        NI, NJ, NK, halo = 70, 40, 5, 4
        eos = EOS_init("WRIGHT")
        tvof = lambda t: dict(T=t[0], S=t[1], eqn_of_state=eos) if neutral else None
        gg = synth.make_grid(NI, NJ, NK, halo=halo, reentrant_x=True, reentrant_y=False, seed=78)
        d = synth.make_dynamics_state(gg, seed=3, umax=0.1, eta_amp=0.2)
        trs = [d["T"], d["S"]]
        rng = np.random.default_rng(11)
        h_ML = np.ascontiguousarray(np.clip(1.2 * rng.random(gg.shape2(_abi.POS_H)) - 0.1, 0.0, None) * d["h"].numpy().sum(0))
        import torch
        h_ML = torch.from_numpy(h_ML)
        params = dict(KHTR=3.0e7, CHECK_DIFFUSIVE_CFL=True, USE_HORIZONTAL_BOUNDARY_DIFFUSION=True, USE_NEUTRAL_DIFFUSION=neutral,
                      NDIFF_INTERIOR_ONLY=neutral)
        dom = Domain(NI, NJ, layout, rank, halo, True, False)
        dg = DeviceGrid(dom.tile_grid(gg))
        dg.set_domain(dom)
        cut = lambda a, pos: dom.cut(a, pos).cuda()
        tr = [cut(t, _abi.POS_H) for t in trs]
        st = tracer_hordiff(cut(d["h"], _abi.POS_H), 3600.0, None, None, dict(h_ML=cut(h_ML, _abi.POS_H)), dg, tracer_hor_diff_init(**params), tr,
                            tv=tvof(tr))
        dg.sync()
        h = halo
        res = [t.cpu().numpy()[:, h:h + dom.nj, h:h + dom.ni] for t in tr]
        np.savez(os.path.join(out_dir, f"tile{rank}.npz"), *res, ij=np.array([dom.i0, dom.j0, dom.ni, dom.nj, st.num_itts]))
        dg.close()
        if rank == 0:      # the one-tile answer
            dg1 = DeviceGrid(gg)
            tr1 = [t.clone().cuda() for t in trs]
            s1 = tracer_hordiff(d["h"].cuda(), 3600.0, None, None, dict(h_ML=h_ML.cuda()), dg1, tracer_hor_diff_init(**params), tr1, tv=tvof(tr1))
            dg1.sync()
            np.savez(os.path.join(out_dir, "global.npz"), *[t.cpu().numpy()[:, h:h + NJ, h:h + NI] for t in tr1], it=np.array([s1.num_itts]))
            dg1.close()
    finally:
        dist.destroy_process_group()
