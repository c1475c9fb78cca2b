"""The kernels and entry points that are one body for both key widths (kat_amd/csrc/kg_device.hpp "one body for both key widths":
k_regrow, k_merge, k_partition, k_get, k_filter and the exports), one scenario at each slot layout side by side: tests/key_widths_case.py,
run with regions of 256 slots so that these small tables have several regions and the one-word ones below k = 32 are packed."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("k,canonical", [(21, True), (32, False), (33, True), (63, False)])      # packed, KV12 with the all-ones k-mer, wide, wide
def test_one_scenario_at_each_key_width(k, canonical):
    env = dict(os.environ, KATGPU_TESTING="1", KATGPU_TEST_REGION_SLOTS="256")
    r = subprocess.run([sys.executable, os.path.join(HERE, "key_widths_case.py"), str(k), "1" if canonical else "0"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "key widths ok: k = %d" % k in r.stdout
