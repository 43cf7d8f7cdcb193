"""The reference's own MOM_tracer_hor_diff.F90 with its MOM_hor_bnd_diffusion.F90 (USE_HORIZONTAL_BOUNDARY_DIFFUSION), compiled unmodified
under tests/fortran/tracer_driver.F90, beside the checker (tests/hbd_checker.py) followed by the unchanged orc.tracer_hordiff: bitwise,
on closed and re-entrant domains.  Build container only (needs the reference and amdflang)."""
import os
import subprocess

import numpy as np
import pytest

import hbd_checker as hc
from helpers import bits_equal, interior
from test_hor_bnd_diffusion import _write_case, case
from test_reference_kernels import FC, REF, build_ref_tracer_driver

pytestmark = [pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src")), reason="the reference is not mounted"),
              pytest.mark.skipif(not os.path.exists(FC), reason="amdflang not present")]

CASES = [("default", {}), ("no_limiter", dict(APPLY_LIMITER=False)), ("limiter_remap", dict(APPLY_LIMITER_REMAP=True)),
         ("linear", dict(HBD_LINEAR_TRANSITION=True)), ("cfl_itts", dict(KhTr=6.0e7, CHECK_DIFFUSIVE_CFL=True)),
         ("neutral_interior", dict(neutral=True))] + \
        [(f"{s}{'_extrap' if e else ''}", dict(HBD_REMAPPING_SCHEME=s, HBD_BOUNDARY_EXTRAP=e)) for s in hc.SCHEMES for e in (False, True)
         if (s, e) != ("PLM", False)]


@pytest.fixture(scope="module")
def tracer_exe(tmp_path_factory):
    return build_ref_tracer_driver(tmp_path_factory.mktemp("ref_tracer_hbd"))


@pytest.mark.parametrize("topo", [(False, False), (True, False)], ids=["closed", "reentrant_x"])
def test_reference_hor_bnd_diffusion_equals_the_checker(tmp_path, tracer_exe, topo):
    g, h, tr, h_ML = case(reentrant=topo)
    bad = []
    for name, kw in CASES:
        ref = _write_case(tmp_path, g, h, tr, h_ML, kw)
        r = subprocess.run([tracer_exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(tmp_path / "params.txt")], capture_output=True, text=True)
        assert r.returncode == 0 and "tracer_driver ok" in r.stdout, (name, r.stdout[-300:], r.stderr[-1500:])
        raw = np.fromfile(str(tmp_path / "out.bin"), dtype="<f8").reshape((len(tr),) + tr[0].shape)
        for m, w in enumerate(ref):
            if not bits_equal(interior(g, raw[m]), interior(g, w)):
                bad.append((name, m, int((interior(g, raw[m]) != interior(g, w)).sum()), float(np.abs(interior(g, raw[m]) - interior(g, w)).max())))
        assert not np.array_equal(interior(g, ref[0]), interior(g, tr[0]))
    assert not bad, bad
