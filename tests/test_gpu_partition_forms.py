"""Every kernel form the partitioned counter dispatches (kat_amd/csrc/kg_count.hip: plan_level1, launch_l2_hb, launch_apply), run on the device
against the oracle: the rows of tests/partition_forms.py -- every k from 12 to 32, both strand modes, every reachable combination of level-1
edition, level-1 item form, level-2 item width and slot layout, each with the segmented level 1 + one-pass level 2 and with both exact
editions (the block rows also with the exact level 2 reading blocks of ten), and the KV12 apply kernels behind the forms that otherwise feed
packed slots (KATGPU_NO_PACKED).  Rows on grids whose level-1 segments cannot hold a round of this size run the exact editions alone
(partition_forms.py: Row.seg); every label of theirs has another row that runs segmented.  A child per region size and kernel editions (tests/partition_forms_case.py: the hooks are read when the
library loads) asserts per row the geometry, the forms the library's trace names for every round, the dump, statistics, histogram and GC
matrix against the oracle's, exactly, and that the direct path took at most 1 % of the k-mers.

The streams (about 930 K bases, and 3.4 M for two rows: tests/partition_forms.py: stream) and the oracle's results per (k, strand mode) are made once
per module, on the CPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import partition_forms as pf
from tests.test_partition_forms_model import LABELS, LABELS_NO_PACKED

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GROUPS = pf.groups()
COMMON = {"KATGPU_TESTING": "1", "KATGPU_TRACE": "1", "KATGPU_PART_MIN_STARTS": "0"}


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    from oracle import koracle as ko
    d = tmp_path_factory.mktemp("partition_forms")
    streams = {"stream": pf.stream(), "long": pf.stream(long=True)}
    streams["short"] = np.ascontiguousarray(streams["stream"][:pf.SHORT_BASES])
    np.save(d / "stream.npy", streams["stream"])
    np.save(d / "long.npy", streams["long"])
    for k, canonical, which in sorted({(r.k, r.canonical, r.which()) for r in pf.ROWS}):
        o = ko.Table(k, canonical).count_bases(streams[which], threads=1 if which == "short" else 8)
        keys, counts = o.dump_sorted()
        for what, a in (("keys", keys), ("counts", counts), ("hist", o.hist()), ("gcp", o.gcp())):
            np.save(d / ("o_%u_%u_%s_%s.npy" % (k, canonical, which, what)), a)
    return str(d)


@pytest.fixture(scope="module")
def children(reference):
    """Runs a group's child once, whichever test asks first: {group id: the child's "row ..." lines}."""
    done = {}

    def run(gid):
        if gid not in done:                                  # (a child that failed is not started again: its failure is kept)
            _, env, st, rows = next(g for g in GROUPS if g[0] == gid)
            r = subprocess.run([sys.executable, os.path.join(HERE, "partition_forms_case.py"), reference, str(st[0]), str(st[1])] + [str(i) for i in rows],
                               env=dict(os.environ, **COMMON, **env), capture_output=True, text=True, timeout=300)
            lines = [line for line in r.stdout.splitlines() if line.startswith("row ")]
            ok = r.returncode == 0 and "partition forms ok: " + " ".join(str(i) for i in rows) in r.stdout
            done[gid] = (lines, None if ok else "exit %d\n" % r.returncode + r.stdout[-3000:] + r.stderr[-4000:])
        lines, failure = done[gid]
        print("\n".join(lines))
        assert failure is None, failure
        return lines
    return run


@pytest.mark.parametrize("gid", [g[0] for g in GROUPS])
def test_forms_match_oracle(children, gid):
    assert children(gid)


def test_every_label_ran(children):
    """Every reachable label is among those the trace named in a segmented, one-pass run -- but for the labels of a table of one level-1 digit, whose
    level 2 and apply are named behind the exact level 1 (partition_forms.py: LABELS_SHORT_ONLY)."""
    seen = set()
    for gid, _, st, _ in GROUPS:
        if st in (pf.FAST, pf.EXACT_L1):
            seen |= {line.split("| label: ")[1].split(" | ")[0] for line in children(gid)}
    print("\n".join(sorted(seen)))
    want = (LABELS | LABELS_NO_PACKED) - pf.LABELS_SHORT_ONLY | {"(exact level 1) " + label.split(" ", 1)[1] for label in pf.LABELS_SHORT_ONLY}
    assert not want - seen, sorted(want - seen)
