"""The block editions of partition levels 1 and 2 (kg_l1_blocks.hpp: k_p1b_scatter, kg_l2_blocks.hpp: k_p2x_fast) on a table that selects
BOTH -- k = 27, canonical, packed slots, 2^15 .. 2^16 regions of 128 slots: 6-byte level-1 items, at most 512 level-1 digits, 5-byte
remainders (the child asserts the widths from the table's geometry: another level-2 edition would also count as a `part_l2` launch) -- forced at sizes the oracle counts in seconds (KATGPU_L1_FAST=2, KATGPU_P2_FAST=2, no minimum of starts).  Every case compares
the table's dump with the oracle's and asserts that the block editions are what ran (tests/block_placing_case.py: the profile's
launches; here: KATGPU_TRACE's "blocks of ten").  The cases are the places where the per-bucket phase and the placing pass take another
path: round and pass boundaries, full segments and an overflowing list, one bucket that takes most of a tile (a tile's worth of blocks from
ONE waiting image, the pool shared out unevenly), streams that end inside and at the edges of a tile.

The reads (300 K of 150 bp from a 2 Mbp genome) and the oracle's dumps are made once per session, on the CPU."""
import os
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
    d = tmp_path_factory.mktemp("block_placing")
    g = synth.genome(2_000_000, seed=31)
    reads = synth.reads(g, 0, 300_000, seed=4)
    np.save(d / "reads.npy", reads)
    o = ko.Table(K, True).count_bases(reads, threads=8)
    keys, counts = o.dump_sorted()
    np.save(d / "keys.npy", keys)
    np.save(d / "counts.npy", counts)
    o.count_bases(np.full(1_000_000, ord("A"), np.uint8))          # (the skew case's stretch ends in an N: no k-mer spans into the reads)
    keys, counts = o.dump_sorted()
    np.save(d / "keys_skew.npy", keys)
    np.save(d / "counts_skew.npy", counts)
    return str(d)


COMMON = {"KATGPU_TESTING": "1", "KATGPU_TRACE": "1", "KATGPU_PART_MIN_STARTS": "0", "KATGPU_L1_FAST": "2", "KATGPU_P2_FAST": "2",
          "KATGPU_TEST_REGION_SLOTS": "128"}


@pytest.mark.parametrize("case,extra", [
    ("plain", {}),
    ("rounds", {"KATGPU_TEST_ROUND_ITEMS": "100000", "KATGPU_TEST_PASS_BUCKETS": "3"}),
    ("full", {"KATGPU_TEST_L1_CPB": "2", "KATGPU_P1_WGS": "1", "KATGPU_TEST_P2_OVF_CAP": "50"}),
    ("skew", {}),
    ("ends", {}),
])
def test_block_editions_match_oracle(reference, case, extra):
    env = dict(os.environ, **COMMON)
    env.update(extra)
    r = subprocess.run([sys.executable, os.path.join(HERE, "block_placing_case.py"), case, reference], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-1500:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "block placing case ok: " + case in r.stdout
    assert "blocks of ten" in r.stderr, r.stderr[-3000:]
