"""The drains of the packed apply's walk (kat_amd/csrc/kg_partition.hpp: ApkWalk::drain_pass, a window of slots per LDS round trip;
kg_apply_lean.hpp: ap_first_event) against the oracle, over probe chains of constructed lengths: a free slot and a match at every distance from
0 to beyond two windows behind the probe rounds, chains that wrap at the region's last slot at every offset of a window, lanes racing for one
free slot (the same new k-mer in 3 and in 64 copies, two new k-mers whose chains end at one slot), regions filled to their last slot with the
free slot at each position of the walk's last window, one k-mer more than a region holds, and chains beyond the lanes' probes (the wave-wide
finish) ending in a claim and in a match -- all in one walk of a table's first sweep, and call by call on a loaded table; walked whole, in
segments of 4096 k-mers, and with the spill hook.  Every chain's length is asserted on the CPU by the case file's linear-probe model.
tests/apply_drain_case.py; a child per set of hooks: they are read when the library loads."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
COMMON = {"KATGPU_TESTING": "1", "KATGPU_TRACE": "1", "KATGPU_PART_MIN_STARTS": "0", "KATGPU_TEST_REGION_SLOTS": "1024", "KATGPU_TEST_LAZY_MIN_SLOTS": "0",
          "KATGPU_TEST_ROUND_ITEMS": "8000000"}


@pytest.mark.parametrize("mode, hooks", [("one", {}), ("seg", {"KATGPU_TEST_AP_SEG": "4096"}), ("spill", {"KATGPU_TEST_SPILL_MOD": "5"})])
def test_chains_of_constructed_lengths_match_oracle(mode, hooks):
    env = {k: v for k, v in os.environ.items() if k not in ("KATGPU_TEST_AP_SEG", "KATGPU_TEST_SPILL_MOD")}
    r = subprocess.run([sys.executable, os.path.join(HERE, "apply_drain_case.py"), mode], capture_output=True, text=True, timeout=90, env=dict(env, **COMMON, **hooks))
    print(r.stdout[-4000:])
    assert r.returncode == 0 and "apply drain ok: " + mode in r.stdout, "exit %d\n" % r.returncode + r.stdout[-3000:] + r.stderr[-4000:]
