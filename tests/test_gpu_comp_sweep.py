"""The fused comparison's sweep of the resident region (kat_amd/csrc/kg_reduce_kernels.hpp: k_comp_fused) tallies the k-mers of count 1 that
the other table lacks per lane; only the others go through the wave's queue and the account.  tests/comp_sweep_case.py builds, per region
size, two packed tables of one grid whose regions hold constructed mixtures of the two kinds (a wave's worth of consecutive slots all of the
first kind, none, one in three, a region the other table holds all of), with and without side-table counts on either side, and compares
both directions of the comparison at several scales and matrix sizes with the oracle, exactly.  A child per region size: the region-size
hook is read when the library loads."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("region_slots", [256, 1024])
def test_sweep_matches_oracle(region_slots):
    r = subprocess.run([sys.executable, os.path.join(HERE, "comp_sweep_case.py"), str(region_slots)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, KATGPU_TESTING="1", KATGPU_TEST_REGION_SLOTS=str(region_slots)))
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "comp sweep ok: %u 42" % region_slots in r.stdout, "exit %d\n" % r.returncode + r.stdout[-3000:] + r.stderr[-4000:]
