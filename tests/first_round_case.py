"""Run in a subprocess by tests/test_gpu_first_round_shape.py (the hooks are read when the library loads): which apply shape a packed table's
first partition round takes (kat_amd/csrc/kg_count.hip: launch_apply).  One stream -- a 40 kb genome sampled at 20x, about 680 K k-mers, in
rounds of at most 400 K -- is counted into a table of 128 K slots, whose first round brings three items per slot and is therefore mostly
repeats: the steady-state shape (`fresh=0` in the trace's "partition forms" line), on slots that no memset has cleared
(KATGPU_TEST_LAZY_MIN_SLOTS=0); and into one of 2 M slots, whose first round could be all new k-mers: inline claims (`fresh=1`).  Every later round says `fresh=0`.
Both tables equal the oracle's: dump, statistics, histogram and GC matrix.

k = 25: with regions of 256 slots a table of 128 K slots has 512 regions, and a 25-mer's remainder behind them (41 bits) still fits a packed
slot; the rule is the packed apply's."""
import atexit
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kat_amd  # noqa: E402
from kat_amd import synth  # noqa: E402
from oracle import koracle as ko  # noqa: E402

K = 25
TRACE = tempfile.NamedTemporaryFile(prefix="first_round_trace_", suffix=".txt")
STDERR = os.dup(2)
os.dup2(TRACE.fileno(), 2)                  # the library's trace lines: looked at per table ...


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


def main():
    assert os.environ["KATGPU_TEST_REGION_SLOTS"] == "256" and int(os.environ["KATGPU_TEST_ROUND_ITEMS"]) == 400_000 and os.environ["KATGPU_TEST_LAZY_MIN_SLOTS"] == "0"
    eng = kat_amd.Engine(0)
    genome = synth.genome(40_000, seed=3)
    bases = synth.reads(genome, 0, 5400, err_ppm=500, seed=1)
    o = ko.Table(K, True).count_bases(bases)
    keys, counts = o.dump_sorted()
    total = int(counts.sum(dtype=np.uint64))
    assert 600_000 < total < 800_000 and keys.size < 70_000, (total, keys.size)
    buf = eng.alloc(bases.size + 32)
    buf.upload(bases)
    for hint, first_fresh in ((128 << 10, 0), (2 << 20, 1)):
        t = eng.table(K, True, size_hint=hint)
        geo = t.geometry()
        assert geo.region_slots == 256 and geo.capacity == hint and t.packed_records(), (hint, geo.region_slots, geo.capacity)
        before = len(forms_lines())
        eng.profile_reset()
        t.count_bases_device(buf.ptr, bases.size)
        prof = eng.profile()
        seen = forms_lines()[before:]
        print("table of %u slots | %s" % (hint, " / ".join(seen)))
        assert t.regrows == 0 and t.geometry().capacity == hint
        assert len(seen) >= 2, seen
        assert all("apply=packed B=512 KP=4 " in line for line in seen), seen
        assert [int(line.rsplit("fresh=", 1)[1].split()[0]) for line in seen] == [first_fresh] + [0] * (len(seen) - 1), (hint, seen)
        assert prof["count"]["units"] <= total // 100, (hint, "direct path", prof["count"]["units"], total)
        gk, gc = t.dump_sorted()
        assert np.array_equal(gk, keys) and np.array_equal(gc, counts), (hint, "dump differs")
        st = t.stats()
        assert st["distinct"] == keys.size and st["total"] == total, (hint, st)
        assert np.array_equal(t.hist(), o.hist()) and np.array_equal(t.gcp(), o.gcp()), (hint, "hist / gcp differ")
        t.free()
    buf.free()
    print("first round ok")


if __name__ == "__main__":
    main()
