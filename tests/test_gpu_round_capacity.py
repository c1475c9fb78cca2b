"""The partition arena sized by the blocked items (kat_amd/csrc/kg_arena_plan.hpp): the level-1 buffer at 6.4 bytes per item where level 1's
block edition runs, a round's capacity by the edition that runs it, the level-2 buffer without the group editions' allowance -- on
tests/test_gpu_block_placing.py's table (k = 27, canonical, packed slots, 2^15 .. 2^16 regions of 128 slots: both block editions), forced at
sizes the oracle counts in seconds.  Every case (tests/round_capacity_case.py, a child process: the hooks are read when the library loads)
compares the table's dump with the oracle's, and under KATGPU_TESTING the library itself checks the guards behind the level-1 buffer, the
level-2 buffer and the overflow list after every round.

The reads (300 K of 150 bp from a 2 Mbp genome) and the oracle's dumps are made once per session, on the CPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
K = 27


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    from kat_amd import synth
    from oracle import koracle as ko
    d = tmp_path_factory.mktemp("round_capacity")
    g = synth.genome(2_000_000, seed=31)
    reads = synth.reads(g, 0, 300_000, seed=4)
    hot = reads.reshape(-1, 151).copy()
    hot[::500] = hot[0]                                              # 600 copies of one read, spread over the stream
    for name, stream in (("", reads), ("_hot", hot.reshape(-1))):
        np.save(d / ("reads%s.npy" % name), stream)
        keys, counts = ko.Table(K, True).count_bases(stream, threads=8).dump_sorted()
        np.save(d / ("keys%s.npy" % name), keys)
        np.save(d / ("counts%s.npy" % name), counts)
    return str(d)


COMMON = {"KATGPU_TESTING": "1", "KATGPU_TRACE": "1", "KATGPU_PART_MIN_STARTS": "0", "KATGPU_L1_FAST": "2", "KATGPU_P2_FAST": "2",
          "KATGPU_TEST_REGION_SLOTS": "128"}
ROUNDS = {"KATGPU_TEST_ROUND_ITEMS": "100000", "KATGPU_TEST_PASS_BUCKETS": "3"}
DONE = {}                                                            # case -> partition rounds of its count


def run_case(reference, case, extra):
    env = dict(os.environ, **COMMON)
    env.update(extra)
    r = subprocess.run([sys.executable, os.path.join(HERE, "round_capacity_case.py"), case, reference], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-1500:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"round capacity case ok: %s rounds=(\d+)" % case, r.stdout)
    assert m, r.stdout[-2000:]
    assert "blocks of ten" in r.stderr and "guard" not in r.stderr, r.stderr[-3000:]
    return int(m.group(1))


@pytest.fixture(scope="module")
def rounds_of_rounds(reference):
    """The `rounds` case, run once: the `fallback` case compares its number of rounds with this one's."""
    if "rounds" not in DONE:
        DONE["rounds"] = run_case(reference, "rounds", ROUNDS)
    return DONE["rounds"]


@pytest.mark.parametrize("case,extra", [
    ("dense", {}),
    ("brim", {"KATGPU_TEST_L1_CPB": "10"}),
    ("brim", {"KATGPU_TEST_L1_CPB": "20"}),
    ("l2_exact", {"KATGPU_TEST_P2_OVF_CAP": "50", "KATGPU_TEST_PASS_BUCKETS": "3"}),
], ids=["dense", "brim-one-block-fallback-then-full-segments", "brim-two-blocks-fallback-then-full-segments", "l2_exact"])
def test_round_capacity_matches_oracle(reference, case, extra):
    assert run_case(reference, case, extra) >= 1


def test_rounds_at_the_new_carve(rounds_of_rounds):
    assert rounds_of_rounds >= 300                                   # 45 M window starts in rounds of at most 100 000 items


def test_fallback_to_the_exact_level_1(reference, rounds_of_rounds):
    """The block round is abandoned; the exact rounds behind it hold at most the exact capacity their trace lines print (the child asserts it),
    and there are more rounds than the block edition made."""
    extra = dict(ROUNDS, KATGPU_TEST_L1_CPB="2", KATGPU_P1_WGS="1", KATGPU_TEST_P2_OVF_CAP="50")
    assert run_case(reference, "fallback", extra) > rounds_of_rounds
