"""The packed apply's walk (kat_amd/csrc/kg_partition.hpp: ApkWalk, with the slot tests and the step of kg_apply_lean.hpp) against the oracle
over what its arithmetic can meet: count fields of 32, 27, 21 and 20 bits, items of 4, 5 and 6 bytes, regions of 256, 4096, 4100 and 9700
slots (the four kernel shapes), a first round with inline claims and loaded rounds without -- and k-mers constructed for its corners: a
remainder of 0 alone and behind nine occupied slots, remainders that differ only in the slot word's high half, a region filled to its last
slot, a count beyond half its range, new k-mers three times in a row in a loaded table.  tests/apply_lean_case.py; a child per round size:
the hooks are read when the library loads."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
COMMON = {"KATGPU_TESTING": "1", "KATGPU_TRACE": "1", "KATGPU_PART_MIN_STARTS": "0", "KATGPU_TEST_REGION_SLOTS": "1024", "KATGPU_TEST_LAZY_MIN_SLOTS": "0"}


@pytest.mark.parametrize("mode, hooks", [("one", {"KATGPU_TEST_ROUND_ITEMS": "8000000"}), ("two", {"KATGPU_TEST_ROUND_ITEMS": "60000", "KATGPU_TEST_AP_SEG": "4096"})])
def test_walk_corners_match_oracle(mode, hooks):
    env = {k: v for k, v in os.environ.items() if k != "KATGPU_TEST_AP_SEG"}
    r = subprocess.run([sys.executable, os.path.join(HERE, "apply_lean_case.py"), mode], capture_output=True, text=True, timeout=300, env=dict(env, **COMMON, **hooks))
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "apply lean ok: " + mode in r.stdout, "exit %d\n" % r.returncode + r.stdout[-3000:] + r.stderr[-4000:]
