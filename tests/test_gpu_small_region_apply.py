"""The packed apply on small regions (kat_amd/csrc/kg_partition.hpp: k_p3_apply_pk; kg_count.hip: apply_pk_shape's `S <= 4096` shapes) and on
the first region size beyond them: tests/small_region_case.py counts a stream of constructed run lengths -- an empty region between two full
ones, one item, exactly one chunk per wave, one item more, a run longer than the waves' first chunks -- into tables whose regions have 256,
3080, 4096 and 4100 slots, in one round from zeros, in two rounds, and by a second call into the same table, and compares the tables and
their comparison with a table of reads against the oracle.  A child per round size: the hooks are read when the library loads."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
COMMON = {"KATGPU_TESTING": "1", "KATGPU_TRACE": "1", "KATGPU_PART_MIN_STARTS": "0", "KATGPU_TEST_REGION_SLOTS": "1024", "KATGPU_TEST_LAZY_MIN_SLOTS": "0"}


@pytest.mark.parametrize("mode, round_items", [("one", 4_000_000), ("two", 70_000)])
def test_small_regions_match_oracle(mode, round_items):
    r = subprocess.run([sys.executable, os.path.join(HERE, "small_region_case.py"), mode], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, **COMMON, KATGPU_TEST_ROUND_ITEMS=str(round_items)))
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "small regions ok: " + mode in r.stdout, "exit %d\n" % r.returncode + r.stdout[-3000:] + r.stderr[-4000:]
