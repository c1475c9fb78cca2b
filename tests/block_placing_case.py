"""Run in a subprocess by tests/test_gpu_block_placing.py (the hooks are read when the library loads): one case of the block editions
of partition levels 1 and 2 (kg_l1_blocks.hpp, kg_l2_blocks.hpp) -- a packed k = 27 table whose geometry selects both (6-byte level-1
items, at most 512 level-1 digits, 5-byte remainders), its dump against the oracle's, and the evidence that the block editions are
what ran, for EVERY count of the case: the profile's launches and KATGPU_TRACE's "blocks of ten" line (the library's stderr goes to
a file that is read back after each count, and on to the parent at the end).

  block_placing_case.py <case> <dir with reads.npy, keys.npy, counts.npy [, keys_skew.npy, counts_skew.npy]>"""
import atexit
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kat_amd  # noqa: E402
from oracle import koracle as ko  # noqa: E402

K = 27
HINT = 8_000_000
TILE_STARTS = 16384 - 32                    # kg_l1_blocks.hpp: window starts of a level-1 tile


TRACE = tempfile.NamedTemporaryFile(prefix="block_placing_trace_", suffix=".txt")
STDERR = os.dup(2)
os.dup2(TRACE.fileno(), 2)                  # the library's trace lines: looked at per count ...


@atexit.register
def _trace_to_parent():                     # ... and handed on
    sys.stderr.flush()
    os.dup2(STDERR, 2)
    with open(TRACE.name) as f:
        sys.stderr.write(f.read())


def trace_lines(what):
    with open(TRACE.name) as f:
        return sum(what in line for line in f)


def count(eng, stream, exact_allowed=False):
    buf = eng.alloc(stream.size + 32)
    buf.upload(stream)
    eng.profile_reset()
    t = eng.table(K, True, size_hint=HINT)
    before = trace_lines("blocks of ten"), trace_lines("exact level")
    t.count_bases_device(buf.ptr, stream.size)
    prof = eng.profile()
    buf.free()
    assert trace_lines("blocks of ten") > before[0], "level 1's block edition did not run"
    assert exact_allowed or trace_lines("exact level") == before[1], "an exact edition took over"
    geo = t.geometry()
    # the geometry the block editions are for: anything else is a failure of the test's set-up, not a reason to skip
    assert 128 <= geo.p1 <= 512 and geo.p2 >= 2 and 64 <= geo.region_slots <= 256, (geo.p1, geo.p2, geo.region_slots)
    # ... and the item widths that select k_p1b_scatter AND k_p2x_fast (kg_count.hip: plan_level1, launch_l2_hb): a level-1 item keeps
    # n1 = 2k - floor(log2 p1) bits, 41 .. 47 of them are 6 bytes; the remainder keeps n1 - log2 p2, 32 .. 39 of them are 5 bytes
    n1 = 2 * K - (geo.p1.bit_length() - 1)
    rb = n1 - (geo.p2.bit_length() - 1)
    assert geo.p2 & (geo.p2 - 1) == 0 and geo.n_regions == geo.p1 * geo.p2 and (1 << 15) <= geo.n_regions <= (1 << 16), (geo.p1, geo.p2, geo.n_regions)
    assert 41 <= n1 <= 47 and 32 <= rb <= 39, (n1, rb)
    assert prof["part_l1_scatter"]["launches"] > 0 and prof["part_l2"]["launches"] > 0 and prof["part_apply"]["launches"] > 0, prof
    return t, prof


def same(t, keys, counts, what):
    gk, gc = t.dump_sorted()
    assert gk.size == keys.size, (what, "distinct", gk.size, keys.size)
    assert np.array_equal(gk, keys), (what, "k-mers differ")
    assert np.array_equal(gc, counts), (what, "counts differ at %d k-mers" % int((gc != counts).sum()))


def direct_share(prof, total, what):
    """What went through the direct kernel: at most what the overflow lists are meant for, 1 % of the input's k-mers."""
    units = prof["count"]["units"]
    print("%s: direct path %d of %d k-mers" % (what, units, total))
    assert units <= 0.01 * total, (what, units, total)


def main():
    case, d = sys.argv[1], sys.argv[2]
    eng = kat_amd.Engine(0)
    reads = np.load(os.path.join(d, "reads.npy"))
    if case in ("plain", "rounds", "full"):
        t, prof = count(eng, reads, exact_allowed=case == "full")
        keys, counts = np.load(os.path.join(d, "keys.npy")), np.load(os.path.join(d, "counts.npy"))
        same(t, keys, counts, case)
        if case != "full":                                 # (full segments and a 50-entry list: the exact editions take over, by design)
            direct_share(prof, int(counts.sum(dtype=np.uint64)), case)
    elif case == "skew":
        stream = np.concatenate([np.full(1_000_000, ord("A"), np.uint8), np.frombuffer(b"N", np.uint8), reads])
        t, prof = count(eng, stream)
        same(t, np.load(os.path.join(d, "keys_skew.npy")), np.load(os.path.join(d, "counts_skew.npy")), case)
    elif case == "ends":
        # shorter than one tile; then streams whose third tile holds 1, 15 and 16 window starts (a tile is 16352 STARTS: a stream of nb bases
        # has nb - K + 1 of them, valid or not), and one that ends with its second tile.  (The whole input first: a process's first partition
        # call sizes the arena, and one sized for a few thousand k-mers has no room for level 1's segments.)
        count(eng, reads)[0].free()
        for nb, tiles in ((9000, 1), (2 * TILE_STARTS + K - 1, 2), (2 * TILE_STARTS + K - 1 + 1, 3), (2 * TILE_STARTS + K - 1 + 15, 3), (2 * TILE_STARTS + K - 1 + 16, 3)):
            assert -(-(nb - K + 1) // TILE_STARTS) == tiles and (tiles < 3 or (nb - K + 1) - 2 * TILE_STARTS in (1, 15, 16)), (nb, tiles)
            stream = np.ascontiguousarray(reads[:nb])
            t, prof = count(eng, stream)
            o = ko.Table(K, True).count_bases(stream)
            same(t, *o.dump_sorted(), (case, nb))
            direct_share(prof, o.total, (case, nb))
            t.free()
    else:
        raise SystemExit("unknown case " + case)
    print("block placing case ok:", case, {k: v["launches"] for k, v in prof.items() if v["launches"]})


if __name__ == "__main__":
    main()
