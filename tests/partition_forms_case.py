"""Run in a subprocess by tests/test_gpu_partition_forms.py (the hooks are read when the library loads): rows of tests/partition_forms.py
that share a region size and the kernel editions.  Per row: the table's geometry against the row's, the stream counted on the device, the
"partition forms" lines of KATGPU_TRACE against the form the row is there for -- one per round, every round, nothing else -- and the table's
dump, statistics, histogram and GC matrix against the oracle's, integer for integer.  What went through the direct kernel is at most 1 % of
the k-mers: a row that the direct path counted would prove nothing.

  partition_forms_case.py <dir with stream.npy, long.npy and the oracle's o_<k>_<canonical>_<stream|long|short>_{keys,counts,hist,gcp}.npy> <l1 fast> <p2 fast> <row> ..."""
import atexit
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kat_amd  # noqa: E402
from tests import partition_forms as pf  # noqa: E402

TRACE = tempfile.NamedTemporaryFile(prefix="partition_forms_trace_", suffix=".txt")
STDERR = os.dup(2)
os.dup2(TRACE.fileno(), 2)                  # the library's trace lines: looked at per row ...


@atexit.register
def _trace_to_parent():                     # ... and handed on
    sys.stderr.flush()
    os.dup2(STDERR, 2)
    with open(TRACE.name) as f:
        sys.stderr.write(f.read())


MARK = "[katgpu] partition forms: "


def forms_lines():
    with open(TRACE.name) as f:
        return [line[len(MARK):].strip() for line in f if line.startswith(MARK)]


def round_lines():
    with open(TRACE.name) as f:
        return sum(line.startswith("[katgpu] partition round") for line in f)


def run_row(eng, d, index, l1_fast, p2_fast):
    row = pf.ROWS[index]
    form = row.form
    assert int(os.environ["KATGPU_TEST_REGION_SLOTS"]) == row.rs and (os.environ.get("KATGPU_NO_PACKED") is not None) == row.no_packed, "the parent's environment is not the row's"
    bases = np.load(os.path.join(d, "long.npy" if row.long else "stream.npy"))
    if row.short:
        bases = np.ascontiguousarray(bases[:pf.SHORT_BASES])
    name = os.path.join(d, "o_%u_%u_%s_" % (row.k, row.canonical, row.which()))
    keys, counts, hist, gcp = (np.load(name + what + ".npy") for what in ("keys", "counts", "hist", "gcp"))
    total = int(counts.sum(dtype=np.uint64))

    buf = eng.alloc(bases.size + 32)        # (the device allocator's alignment: nothing but overflow goes through the direct path)
    assert buf.ptr % 16 == 0
    buf.upload(bases)
    t = eng.table(row.k, row.canonical, size_hint=row.hint)

    def geometry_is_the_rows():
        geo = t.geometry()
        assert (geo.p1, geo.p2, geo.region_slots, geo.n_regions) == (form.p1, form.p2, form.region_slots, form.n_regions), (row, geo.p1, geo.p2, geo.region_slots, geo.n_regions)
        assert t.slot_bytes() == form.slot_bytes, (row, t.slot_bytes())
    geometry_is_the_rows()
    before, rounds = len(forms_lines()), round_lines()
    eng.profile_reset()
    t.count_bases_device(buf.ptr, bases.size)
    prof = eng.profile()
    buf.free()
    assert t.regrows == 0, (row, "the table grew: its geometry is no longer the row's")
    geometry_is_the_rows()

    seen, rounds = forms_lines()[before:], round_lines() - rounds
    expected = [form.trace(l1_fast, p2_fast, fresh=True)] + [form.trace(l1_fast, p2_fast, fresh=False)] * (len(seen) - 1)
    share = prof["count"]["units"] / total
    # (one line per row for the parent's report; the label of a segmented round is what test_every_label_ran collects)
    label = "nothing" if not seen else pf.label_of_trace(seen[0]) if l1_fast else "(exact level 1) " + pf.label_of_trace(seen[0]).split(" ", 1)[1]
    print("row %u | %s | expected: %s | seen: %s | label: %s | rounds %u | direct path %u of %u k-mers = %.3f %%" % (
        index, row, form.trace(l1_fast, p2_fast, fresh=True), " / ".join(sorted(set(seen))) or "nothing", label, len(seen), prof["count"]["units"], total, 100 * share))
    assert seen and (row.short or len(seen) >= 2) and len(seen) == rounds, (row, "partition rounds", rounds, "of them with their forms named", len(seen))
    assert seen == expected, (row, seen, expected)
    if l1_fast:
        assert row.seg and label == row.label, (row, label)
    assert prof["part_l1_scatter"]["launches"] >= len(seen) and prof["part_l2"]["launches"] >= len(seen) and prof["part_apply"]["launches"] >= len(seen), (row, prof)
    assert share <= 0.01, (row, "direct path", prof["count"]["units"], total)

    gk, gc = t.dump_sorted()
    assert gk.size == keys.size, (row, "distinct", gk.size, keys.size)
    assert np.array_equal(gk, keys), (row, "k-mers differ")
    assert np.array_equal(gc, counts), (row, "counts differ at %d k-mers" % int((gc != counts).sum()))
    st = t.stats()
    assert st["distinct"] == keys.size and st["total"] == total, (row, st, keys.size, total)
    assert np.array_equal(t.hist(), hist), (row, "hist differs")
    assert np.array_equal(t.gcp(), gcp), (row, "gcp differs")
    t.free()


def main():
    d, l1_fast, p2_fast = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    assert int(os.environ["KATGPU_L1_FAST"]) == l1_fast and int(os.environ["KATGPU_P2_FAST"]) == p2_fast
    eng = kat_amd.Engine(0)
    for index in map(int, sys.argv[4:]):
        run_row(eng, d, index, l1_fast, p2_fast)
    print("partition forms ok:", " ".join(sys.argv[4:]))


if __name__ == "__main__":
    main()
