"""Run in a subprocess by tests/test_gpu_reducer_forms.py with KATGPU_* hooks in the environment: katgpu_hist and katgpu_gcp on the
tables of tests/reducer_forms_model.py (crafted records through merge_host / merge_host_wide, and a counted stream), every argument
of the case lists, every result equal to both the model's and the oracle's (made once by the parent: argv[1]).  Every call's
"reducer form:" trace line must name what the model's dispatch says; the forms seen are printed for the parent's coverage check.

argv: the reference directory, then the layouts to run."""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kat_amd  # noqa: E402
from oracle import koracle as ko  # noqa: E402
from tests import reducer_forms_model as rf  # noqa: E402

PLAIN_INC = os.environ.get("KATGPU_COMP_PLAIN_INC", "1") != "0"
NO_PACKED = "KATGPU_NO_PACKED" in os.environ
REGION_SLOTS = int(os.environ["KATGPU_TEST_REGION_SLOTS"])


class Trace:
    """The library's stderr, in a file: take() gives the "reducer form:" lines written since the last take()."""

    def __init__(self):
        self.keep = os.dup(2)
        self.f = tempfile.TemporaryFile()
        os.dup2(self.f.fileno(), 2)
        self.pos = 0

    def take(self):
        size = os.fstat(self.f.fileno()).st_size
        text = os.pread(self.f.fileno(), size - self.pos, self.pos).decode(errors="replace")
        self.pos = size
        return [line.split("reducer form: ", 1)[1].split() for line in text.splitlines() if "reducer form: " in line]

    def restore(self, show):
        """stderr as it was; show: with the tail of what the file took."""
        os.dup2(self.keep, 2)
        size = os.fstat(self.f.fileno()).st_size
        if show:
            os.write(2, os.pread(self.f.fileno(), min(size, 6000), max(0, size - 6000)))


def fields(words):
    return {w.split("=")[0]: int(w.split("=")[1]) for w in words if "=" in w}


def dense(ref, name, shape):
    out = np.zeros(int(np.prod(shape)), np.uint64)
    out[ref[name + "_idx"]] = ref[name + "_val"]
    return out.reshape(shape)


def run_layout(eng, trace, refdir, la, seen):
    assert la.region_slots == REGION_SLOTS, (la, REGION_SLOTS)
    slot_bytes = 12 if NO_PACKED and la.k <= 32 else la.slot_bytes
    n_regions, cbits = rf.table_geometry(la.k, la.size_hint, la.region_slots, packed=not NO_PACKED)
    ref = np.load(os.path.join(refdir, la.name + ".npz"))
    stream = np.load(os.path.join(refdir, "stream.npy"))
    n_calls = 0
    for twin in ("a", "b"):
        t = eng.table(la.k, False, size_hint=la.size_hint).count_bases(stream)
        hi, lo, counts = (ref["%s_%s" % (twin, x)] for x in ("hi", "lo", "counts"))
        if la.k > 32:
            t.merge_host_wide(hi, lo, counts)
        else:
            t.merge_host(lo, counts)
        assert t.slot_bytes() == slot_bytes, (la.name, t.slot_bytes())
        st = t.stats(want_total=False)
        capacity = st["capacity"]
        assert (capacity, t.regrows, st["distinct"]) == (n_regions * la.region_slots, 0, int(ref[twin + "_distinct"])), (la.name, st, t.regrows)
        if la.k <= 32:                                              # (a wide table has no geometry to ask for: its regions follow from the capacity)
            g = t.geometry()
            assert (g.n_regions, g.region_slots) == (n_regions, la.region_slots), (la.name, g.n_regions, g.region_slots)
        trace.take()
        for i, (low, high, inc) in enumerate(rf.HIST_TRIPLES):
            got = t.hist(low, high, inc)
            base, ceil, nb = rf.hist_geometry(low, high)
            (words,) = trace.take()
            f = fields(words)
            assert words[:2] == ["hist", rf.hist_kernel(slot_bytes)] and (f["lds_bins"], f["nb"]) == (rf.hist_lds_bins(nb), nb), (la.name, twin, words)
            assert (f["n_ovf"] != 0) == (twin == "b") and 1 <= f["grid"] <= max(1, -(-capacity // 4096)), (la.name, twin, words)
            for who in ("model", "oracle"):
                assert np.array_equal(got, dense(ref, "%s_hist%d_%s" % (twin, i, who), (nb,))), (la.name, twin, low, high, inc, who)
            seen.add(("hist", words[1], "global" if nb > f["lds_bins"] else "lds", twin == "b"))
            n_calls += 1
        for i, (scale, bins) in enumerate(rf.gcp_args(la.k, twin)):
            got = t.gcp(scale, bins)
            (words,) = trace.take()
            f = fields(words)
            want = rf.dispatch(la.k, slot_bytes, bins, PLAIN_INC)
            assert words[:2] == ["gcp", want.kernel] and (f["use_lds"], f["per_cu"], f["lds"], f["cbits"]) == (want.use_lds, want.per_cu, want.lds, cbits), (la.name, twin, scale, bins, words, want)
            assert (f["n_ovf"] != 0) == (twin == "b") and f["grid"] >= 1, (la.name, twin, words)
            if want.kernel == "pk":
                assert f["grid"] <= -(-n_regions // rf.SCAN_WAVES)
                if la.name == "pkmany":                             # a second region per wave, in both grid sizes
                    assert n_regions > f["grid"] * rf.SCAN_WAVES, (n_regions, words)
                    if want.per_cu == 2:
                        seen.add(("gcp", "pk", "second region per wave", twin == "b"))
                if la.region_slots // 4 > 64:
                    seen.add(("gcp", "pk", "second round of quads", twin == "b"))
            for who in ("model", "oracle"):
                assert np.array_equal(got, dense(ref, "%s_gcp%d_%s" % (twin, i, who), (la.k, bins + 1))), (la.name, twin, scale, bins, who, words)
            seen.add(("gcp", want.kernel, want.use_lds, twin == "b"))
            n_calls += 1
        t.free()
    return n_calls


def run_uncleared(eng, trace):
    """hist and gcp as the first kernels on a new packed table (left uncleared under KATGPU_TEST_LAZY_MIN_SLOTS=1), then after a first merge."""
    k = rf.LAZY_K
    t = eng.table(k, False, size_hint=rf.LAZY_HINT)
    h, g = t.hist(), t.gcp()
    assert not h.any() and not g.any() and h.shape == (10001,) and g.shape == (k, 1001)
    t.free()
    t = eng.table(k, False, size_hint=rf.LAZY_HINT)
    g, h = t.gcp(0.37, 2000), t.hist(1, 100000, 7)
    assert not h.any() and not g.any()
    assert t.slot_bytes() == (12 if NO_PACKED else 8)
    keys, counts = zip(*rf.LAZY_KEYS)
    t.merge_host(keys, counts)
    o = ko.Table(k, False)
    for key, c in rf.LAZY_KEYS:
        o.add(key, c)
    m = rf.Multiset(k, list(rf.LAZY_KEYS))
    n = 0
    for low, high, inc in ((1, 10000, 1), (1, 100000, 7)):
        got = t.hist(low, high, inc)
        assert np.array_equal(got, o.hist(low, high, inc)) and np.array_equal(got, rf.hist_model(m, *rf.hist_geometry(low, high)[:2], inc, got.size))
        n += 1
    for scale, bins in ((1.0, 1000), (0.37, 2000), (3.0, 5000)):
        got = t.gcp(scale, bins)
        assert np.array_equal(got, o.gcp(scale, bins)) and np.array_equal(got, rf.gcp_model(m, k, scale, bins))
        n += 1
    t.free()
    trace.take()
    return n + 4


def main():
    refdir, names = sys.argv[1], sys.argv[2:]
    trace = Trace()
    done = False
    try:
        eng = kat_amd.Engine(0)
        seen, n = set(), 0
        n += run_uncleared(eng, trace)
        for name in names:
            n += run_layout(eng, trace, refdir, rf.LAYOUT[name], seen)
        done = True
    finally:
        trace.restore(show=not done)
    print("forms seen: " + json.dumps(sorted((list(f) for f in seen), key=str)))
    print("reducer forms ok: %s, %d calls" % (" ".join(names), n))


if __name__ == "__main__":
    main()
