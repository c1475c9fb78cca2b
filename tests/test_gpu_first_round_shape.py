"""A packed table's first partition round claims its new k-mers inside the probe rounds only where the round can be mostly new k-mers: fewer items
than the table has slots (kat_amd/csrc/kg_count.hip: launch_apply).  A deep library's first round -- more items than slots -- takes the
steady-state shape.  tests/first_round_case.py counts one stream into a table of each kind, reads the shapes from the trace and compares the
tables with the oracle.  A child process: the hooks are read when the library loads."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ENV = {"KATGPU_TESTING": "1", "KATGPU_TRACE": "1", "KATGPU_PART_MIN_STARTS": "0", "KATGPU_TEST_REGION_SLOTS": "256", "KATGPU_TEST_ROUND_ITEMS": "400000",
       "KATGPU_TEST_LAZY_MIN_SLOTS": "0"}       # (no table is cleared when it is made: both shapes' first sweep starts its regions from zeros over whatever the memory held)


def test_first_round_shape_follows_items_per_slot():
    r = subprocess.run([sys.executable, os.path.join(HERE, "first_round_case.py")], capture_output=True, text=True, timeout=300, env=dict(os.environ, **ENV))
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "first round ok" in r.stdout, "exit %d\n" % r.returncode + r.stdout[-3000:] + r.stderr[-4000:]
