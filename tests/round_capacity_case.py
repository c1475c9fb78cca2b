"""Run in a subprocess by tests/test_gpu_round_capacity.py (the hooks are read when the library loads): one case of the partition arena that
is sized by the blocked items (kat_amd/csrc/kg_arena_plan.hpp) -- the level-1 buffer at 6.4 bytes per item where the block edition runs, a
round's capacity by the edition that runs it, the level-2 buffer without the group editions' allowance.  tests/block_placing_case.py's
geometry and inputs (k = 27 canonical, 128-slot regions, hint 8 M, 300 K reads of a 2 Mbp genome); every count is compared with the oracle's
dump, and under KATGPU_TESTING the library checks the guards behind its three buffers after every round: a kernel that wrote beyond one
fails the call.

  round_capacity_case.py <case> <dir with reads.npy, keys.npy, counts.npy, reads_hot.npy, keys_hot.npy, counts_hot.npy>

(reads_hot: the reads with every 500th replaced by the first -- 124 k-mers that arrive 600 times more often than a run has room for, spread over
the whole stream: level 1's segments hold them, the one-pass level 2's runs do not.)

Every case first counts the reads as they are.  `brim` is TWO experiments: that first count runs against segments of one or two blocks
(KATGPU_TEST_L1_CPB), where nearly every k-mer is beyond its segment, the default list does not hold and the exact level 1 takes over inside a
buffer carved for 6.4-byte items (a fallback, asserted); its trace line tells the workgroups, from which the second count's stream is made --
reads spaced by stretches of N so that segments are full to the brim beside each other in neighbouring buckets while the k-mers beyond them fit
the default list: THAT count is the one without an exact fallback.
`fallback` cannot tell the exact level 1's capacity from the block edition's at this size: the buffer's fixed part (SEG_PAD per workgroup and
bucket) gives the exact layout room for all of KATGPU_TEST_ROUND_ITEMS, so it checks that the abandoned round is repeated exactly, that no exact
round exceeds the capacity its line prints, and the dump; that exact rounds behind a fallback are planned at 8 bytes per item is checked by
tests/native/arena_plan_check.cc (exact_items, config 4's three exact rounds) and, at run time, by level1()'s host check, which fails the call.

Prints "round capacity case ok: <case> rounds=<partition rounds of the last count>"."""
import atexit
import os
import re
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kat_amd  # noqa: E402
from oracle import koracle as ko  # noqa: E402

K = 27
HINT = 8_000_000
READ = 151                                  # bytes of a read in the stream (150 bases and a separator)
TILE_STARTS = 16384 - 32                    # kg_l1_blocks.hpp: window starts of a level-1 tile

TRACE = tempfile.NamedTemporaryFile(prefix="round_capacity_trace_", suffix=".txt")
STDERR = os.dup(2)
os.dup2(TRACE.fileno(), 2)                  # the library's trace lines: looked at per count ...


@atexit.register
def _trace_to_parent():                     # ... and handed on
    sys.stderr.flush()
    os.dup2(STDERR, 2)
    with open(TRACE.name) as f:
        sys.stderr.write(f.read())


def trace():
    with open(TRACE.name) as f:
        return f.read().splitlines()


SEG = re.compile(r"partition round \(segmented level 1, blocks of ten\): (\d+) starts, ~(\d+) items, (\d+) k-mers per segment \(arena [\d.]+ GB; capacity (\d+) items, (\w+), stride (\d+)\)")
EXACT = re.compile(r"partition round: (\d+) starts -> (\d+) items \(buffer (\d+) items, arena [\d.]+ GB, ratio [\d.]+; capacity (\d+) items, (\w+), stride (\d+)\)")


def count(eng, stream):
    """One count of `stream` into a fresh table: (table, profile, this count's trace lines)."""
    buf = eng.alloc(stream.size + 32)
    buf.upload(stream)
    eng.profile_reset()
    t = eng.table(K, True, size_hint=HINT)
    before = len(trace())
    t.count_bases_device(buf.ptr, stream.size)
    prof = eng.profile()
    buf.free()
    geo = t.geometry()
    # the geometry that selects both block editions (tests/block_placing_case.py): anything else is a failure of the test's set-up
    n1 = 2 * K - (geo.p1.bit_length() - 1)
    rb = n1 - (geo.p2.bit_length() - 1)
    assert 128 <= geo.p1 <= 512 and geo.p2 & (geo.p2 - 1) == 0 and geo.n_regions == geo.p1 * geo.p2 and 41 <= n1 <= 47 and 32 <= rb <= 39, (geo.p1, geo.p2, geo.n_regions)
    return t, prof, trace()[before:]


def same(t, keys, counts, what):
    gk, gc = t.dump_sorted()
    assert gk.size == keys.size, (what, "distinct", gk.size, keys.size)
    assert np.array_equal(gk, keys), (what, "k-mers differ")
    assert np.array_equal(gc, counts), (what, "counts differ at %d k-mers" % int((gc != counts).sum()))


def segmented(lines):
    return [tuple(int(x) if x.isdigit() else x for x in m.groups()) for m in map(SEG.search, lines) if m]


def exact(lines):
    return [tuple(int(x) if x.isdigit() else x for x in m.groups()) for m in map(EXACT.search, lines) if m]


def dense_stride(line, what):
    """A block round's trace line: the stride is the segments' blocks -- workgroups x blocks x 64 bytes + one block -- not 8 bytes per k-mer.  Returns the workgroups."""
    starts, items, seg_cap, cap, edition, stride = line
    assert edition == "Blocks" and seg_cap % 10 == 0 and stride % 64 == 0, (what, line)
    wgs, rest = divmod(stride - 64, seg_cap // 10 * 64)
    assert rest == 0 and wgs >= 1 and stride < 8 * wgs * seg_cap, (what, "not the dense stride", line)
    assert items <= cap, (what, "a round beyond its capacity", line)
    return wgs


def has(lines, what):
    return sum(what in line for line in lines)


def main():
    case, d = sys.argv[1], sys.argv[2]
    eng = kat_amd.Engine(0)
    hot = "_hot" if case == "l2_exact" else ""
    reads = np.load(os.path.join(d, "reads%s.npy" % hot))
    keys, counts = np.load(os.path.join(d, "keys%s.npy" % hot)), np.load(os.path.join(d, "counts%s.npy" % hot))
    total = int(counts.sum(dtype=np.uint64))
    t, prof, lines = count(eng, reads)
    same(t, keys, counts, case)
    seg, ex = segmented(lines), exact(lines)
    rounds = has(lines, "[katgpu] partition round")
    assert seg, "level 1's block edition did not run"
    if case == "dense":
        assert len(seg) == 1 and not ex and not has(lines, "exact level"), lines
        dense_stride(seg[0], case)
        assert prof["count"]["units"] <= 0.01 * total, (case, "direct path", prof["count"]["units"], total)
    elif case == "rounds":
        assert int(os.environ["KATGPU_TEST_ROUND_ITEMS"]) == 100_000 and os.environ["KATGPU_TEST_PASS_BUCKETS"] == "3"
        assert len(seg) == rounds and rounds >= reads.size // 100_000 and not has(lines, "exact level"), (rounds, len(seg))
        for line in seg:
            dense_stride(line, case)
            assert line[3] == 100_000, (case, "capacity", line)
        assert has(lines, "passes of 3 buckets") == rounds, (case, "passes")
        assert prof["count"]["units"] <= 0.01 * total, (case, "direct path", prof["count"]["units"], total)
    elif case == "brim":
        # The first count (above) ran against segments of one or two blocks: all but a tenth of its k-mers were beyond them, the list did not hold,
        # the exact level 1 took over -- in a buffer carved for 6.4-byte items -- and the dump is the oracle's.  Its trace line tells the workgroups.
        cpb = int(os.environ["KATGPU_TEST_L1_CPB"])
        assert cpb in (10, 20) and has(lines, "exact level 1 from here on") == 1 and seg[0][2] == cpb, lines[:4]
        wgs = dense_stride(seg[0], case)
        assert ex and all(line[1] <= line[3] and line[4].startswith("Exact") for line in ex), ex
        p1 = t.geometry().p1
        t.free()
        # Now a stream whose segments are full to the brim, NEXT TO EACH OTHER in neighbouring buckets, but whose k-mers beyond them fit the default list:
        # every workgroup gets two tiles, and a segment 0.6 of its capacity in k-mers on average (a Poisson number: one segment in twenty is full, about a
        # k-mer in a hundred is beyond its segment).  Reads of 150 bases, each followed by a stretch of N: window starts without a k-mer.
        n_starts = 2 * wgs * TILE_STARTS
        n_reads = int(0.6 * cpb * wgs * p1 / (150 - K + 1))
        assert n_reads * READ <= reads.size and n_reads * 2 * READ <= n_starts, (n_reads, n_starts)
        gap = n_starts // n_reads
        stream = np.full((n_reads, gap), ord("N"), np.uint8)
        stream[:, :150] = reads.reshape(-1, READ)[:n_reads, :150]
        stream = stream.reshape(-1)
        o = ko.Table(K, True).count_bases(stream)
        t, prof, lines = count(eng, stream)
        same(t, *o.dump_sorted(), (case, "sparse"))
        seg, rounds = segmented(lines), has(lines, "[katgpu] partition round")
        assert len(seg) == 1 and seg[0][2] == cpb and not has(lines, "exact level"), lines
        dense_stride(seg[0], (case, "sparse"))
        units = prof["count"]["units"]
        print("brim: %d k-mers, %d workgroups x %d buckets x %d: direct path %d" % (o.total, wgs, p1, cpb, units))
        assert 0 < units <= 0.03 * o.total, (case, "k-mers beyond their segments", units, o.total)      # (some segments WERE full; the list held)
    elif case == "fallback":
        # the block round is abandoned (segments of one block, a list of 50); every exact round behind it holds at most the exact capacity of its line,
        # which is below the block edition's: the caller compares the number of rounds with the `rounds` case's
        assert int(os.environ["KATGPU_TEST_ROUND_ITEMS"]) == 100_000 and os.environ["KATGPU_TEST_L1_CPB"] == "2" and os.environ["KATGPU_TEST_P2_OVF_CAP"] == "50"
        assert len(seg) == 1 and has(lines, "exact level 1 from here on") == 1, (len(seg), lines[:4])
        dense_stride(seg[0], case)
        assert seg[0][3] == 100_000 and ex and len(ex) == rounds - 1, (seg[0], len(ex), rounds)
        # (at this size the buffer's fixed part -- SEG_PAD per workgroup and bucket -- gives the exact layout room for all of KATGPU_TEST_ROUND_ITEMS: the
        # capacities differ from 64 M k-mers per round on, tests/native/arena_plan_check.cc; the abandoned round is what makes the rounds more)
        for starts, items, buffer, cap, edition, stride in ex:
            assert edition.startswith("Exact") and stride == 0 and items <= cap <= 100_000, (case, "an exact round", starts, items, buffer, cap)
    elif case == "l2_exact":
        assert os.environ["KATGPU_TEST_P2_OVF_CAP"] == "50" and os.environ["KATGPU_TEST_PASS_BUCKETS"] == "3" and "KATGPU_TEST_ROUND_ITEMS" not in os.environ
        assert len(seg) == 1 and not ex and has(lines, "exact level 2 from here on") == 1 and not has(lines, "exact level 1"), lines[:6]
        dense_stride(seg[0], case)
        assert has(lines, "l2=blocks+exact"), [line for line in lines if "partition forms" in line]
    else:
        raise SystemExit("unknown case " + case)
    print("round capacity case ok: %s rounds=%d" % (case, rounds))


if __name__ == "__main__":
    main()
