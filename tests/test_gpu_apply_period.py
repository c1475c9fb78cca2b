"""The packed apply's region loop (kat_amd/csrc/kg_partition.hpp: k_p3_apply_pk) against the oracle: the next region's loads leave with
the wave that has finished the run, the fill takes them from registers, the write-back brings the counters back to the invariant -- over
runs of 0, 1, a chunk and half a chunk give or take one k-mer, one chunk per wave give or take a chunk and one k-mer, and two per wave and
a half, in regions whose neighbours along the workgroup's stride are empty, four of them followed on the stride by loaded regions behind empty
ones (the words the early loads bring are the ones the next fill uses); as a table's first sweep and on a loaded table (claims
through the queues: the same new k-mer in several lanes, two new k-mers with one home slot, a wrap at the region's last slot, a region
filling up), walked whole, in segments of 4096 k-mers, and with the spill hook; a count beyond half its range in a run's last segment.
tests/apply_period_case.py; a child per set of hooks: they are read when the library loads."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
COMMON = {"KATGPU_TESTING": "1", "KATGPU_TRACE": "1", "KATGPU_PART_MIN_STARTS": "0", "KATGPU_TEST_REGION_SLOTS": "1024", "KATGPU_TEST_LAZY_MIN_SLOTS": "0",
          "KATGPU_TEST_ROUND_ITEMS": "8000000"}


@pytest.mark.parametrize("mode, hooks", [("one", {}), ("seg", {"KATGPU_TEST_AP_SEG": "4096"}), ("spill", {"KATGPU_TEST_SPILL_MOD": "5"})])
def test_runs_of_chosen_lengths_match_oracle(mode, hooks):
    env = {k: v for k, v in os.environ.items() if k not in ("KATGPU_TEST_AP_SEG", "KATGPU_TEST_SPILL_MOD")}
    r = subprocess.run([sys.executable, os.path.join(HERE, "apply_period_case.py"), mode], capture_output=True, text=True, timeout=60, env=dict(env, **COMMON, **hooks))      # (1.2 to 1.4 s per case on an MI355X)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "apply period ok: " + mode in r.stdout, "exit %d\n" % r.returncode + r.stdout[-3000:] + r.stderr[-4000:]
