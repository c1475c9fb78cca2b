"""Per-record coverage statistics on the device: katgpu_table_record_stats_host / _device (kg_record_stats.hpp) against
tests/record_stats_model.py, field by field and exactly -- key widths, the short / long limit, batch boundaries, the device form,
counts beyond 32 bits, heavy ties, argument errors -- and `katgpu cold` / `katgpu sect -n` end to end with per-position profiles
forbidden."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kat_amd
from tests import record_stats_case as case
from tests import record_stats_model as rm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kat_amd", "bin", "katgpu")


def _oracle(ko, k, canonical):
    return (ko.WideTable(k, canonical) if k > 32 else ko.Table(k, canonical)).count_bases(case.counted(k))


def _assert_equal(got, want, what=""):
    assert got.dtype == rm.DTYPE and got.shape == want.shape
    for f in rm.FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, (what, f, bad[:5], got[f][bad[:5]], want[f][bad[:5]])


def _in_child(kind, k, canonical, tmp_path, tag, **env):
    out = str(tmp_path / (tag + ".npy"))
    e = dict(os.environ)
    e.update({name: str(v) for name, v in env.items()})
    r = subprocess.run([sys.executable, "-m", "tests.record_stats_case", kind, str(k), str(int(canonical)), out], cwd=ROOT, env=e,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    _in_child.sections = int(open(out + ".sections").read())
    return np.load(out)


@pytest.mark.parametrize("k,canonical", [(5, True), (5, False), (17, True), (17, False), (27, True), (27, False), (32, True), (32, False),
                                         (33, True), (51, False), (63, True)])
def test_key_widths_and_flags(engine, ko, k, canonical):
    b, st, ln = case.mix(k)
    t = engine.table(k, canonical).count_bases(case.counted(k))
    if k in (17, 27):
        assert t.slot_bytes() == (8 if k == 17 else 12)             # both layouts of a one-word table
    o = _oracle(ko, k, canonical)
    assert (ln > 960 + k).any() and (ln < 300).any()                # both kernels run
    for canonicalise in (canonical, not canonical):
        counts, _ = ko.profile(o, b.tobytes(), canonicalise)
        want = rm.record_stats(b, st, ln, k, counts)
        assert int(want["median"].max()) >= 3 and len(set(want["median"].tolist())) >= 3 and int(want["invalid"].sum()) > 0
        _assert_equal(t.record_stats(b, st, ln, canonicalise), want, (k, canonicalise))
    t.free()


def test_short_long_limit(ko, tmp_path):
    """The same records all-short (the default limit: none has more than 960 windows), all-long and mixed."""
    k = 21
    b, st, ln = case.mix(k, contigs=False)
    counts, _ = ko.profile(_oracle(ko, k, True), b.tobytes(), True)
    want = rm.record_stats(b, st, ln, k, counts)
    got, sections = [], []
    for lim in (None, 0, 100):
        got.append(_in_child("reads", k, True, tmp_path, "lim%s" % lim, **({} if lim is None else {"KATGPU_TEST_STATS_SHORT": lim})))
        sections.append(_in_child.sections)
    # the hook bites: one batch, so one timed section of the short kernel, and a second one when any record goes the long way
    assert sections == [1, 2, 2] and (ln > 100 + k).any() and (ln < 100).any()
    for g in got:
        _assert_equal(g, want)
        assert np.array_equal(g, got[0])


def test_batch_boundaries(engine, ko, tmp_path):
    k = 21
    b, st, ln = case.mix(k, empties=5000)
    counts, _ = ko.profile(_oracle(ko, k, True), b.tobytes(), True)
    want = rm.record_stats(b, st, ln, k, counts)
    # batches of 20000 bases: smaller than the contigs, larger than the reads; the 5000 empty records at the end make a batch
    _assert_equal(_in_child("mix", k, True, tmp_path, "batch", KATGPU_TEST_STATS_BATCH=20000), want)
    # the same with nearly every record long: a batch also ends where its long records reach 5000 windows between them
    _assert_equal(_in_child("mix", k, True, tmp_path, "batchlong", KATGPU_TEST_STATS_BATCH=20000, KATGPU_TEST_STATS_SHORT=50), want)
    assert _in_child.sections > 100
    # one record beyond the default batch of 2^25 bases: a periodic tiling of the genome, so one period of counts serves the model
    g = case.genome(k)
    big = np.tile(g, 170)[: (33 << 20) + 12345]
    t = engine.table(k, True).count_bases(case.counted(k))
    period, _ = ko.profile(_oracle(ko, k, True), np.concatenate([g, g[: k - 1]]).tobytes(), True)
    nb = big.size - k + 1
    tail = b"NN" + g[5000:5200].tobytes()
    buf = np.concatenate([big, np.frombuffer(tail, np.uint8)])
    got = t.record_stats(buf, [0, big.size + 2], [big.size, 200])
    _assert_equal(got[:1], rm.record_stats(big, [0], [big.size], k, period[np.arange(nb) % g.size]))
    _assert_equal(got[1:], rm.record_stats(g[5000:5200], [0], [200], k, period[5000:5200]))
    t.free()


def test_long_scratch_follows_the_long_records(engine):
    """A full batch of reads with one record just past the limit: the count scratch is that record's windows, not the batch's (8
    bytes x 2^25 would stay parked in the context's pool, which keeps blocks from 64 MiB on)."""
    k = 21
    g = case.genome(k)
    t = engine.table(k, True).count_bases(case.counted(k))
    bases = np.tile(g, 166)[:33_000_000]
    st = np.append(np.arange(0, 32_000_000, 151, dtype=np.uint64), np.uint64(32_500_000))
    ln = np.append(np.full(st.size - 1, 150, np.uint64), np.uint64(1000 + k - 1))
    engine.release_scratch()
    free0, _ = engine.mem_info()
    got = t.record_stats(bases, st, ln)
    free1, _ = engine.mem_info()
    assert free0 - free1 < (64 << 20), (free0, free1)
    alone = t.record_stats(bases[32_500_000:32_500_000 + 1000 + k - 1], [0], [1000 + k - 1])
    assert got[-1] == alone[0] and int(alone["non_zero"][0]) > 500                 # (1 % junk bytes: a fifth of the 21-base windows is invalid)
    assert np.array_equal(got[:5], t.record_stats(bases[:755], st[:5], ln[:5]))
    t.free()


def test_device_form(engine, ko):
    k = 21
    b, st, ln = case.mix(k)
    t = engine.table(k, True).count_bases(case.counted(k))
    counts, _ = ko.profile(_oracle(ko, k, True), b.tobytes(), True)
    want = rm.record_stats(b, st, ln, k, counts)
    m = st.size
    for shift in (0, 1, 7, 16):
        db = engine.alloc(b.size + 64)
        db.upload(b, offset=shift)
        dr = engine.alloc(8 * 8 * m)
        dr.upload(st)
        dr.upload(ln, offset=8 * m)
        t.record_stats_device(db.ptr + shift, b.size, dr.ptr, dr.ptr + 8 * m, m, dr.ptr + 16 * m)
        engine.sync()
        got = dr.download(np.uint64, 6 * m, offset=16 * m).view(rm.DTYPE)
        _assert_equal(got, want, shift)
        db.free(); dr.free()
    t.free()


def _big_want(ko):
    o = ko.Table(9, False)
    _, keys, counts = case.big_keys(ko)
    for key, c in zip(keys, counts):
        o.add(key, c)
    b, st, ln = case.big_records()
    prof, _ = ko.profile(o, b.tobytes(), False)
    return b, st, ln, rm.record_stats(b, st, ln, 9, prof)


def test_large_counts(engine, ko, tmp_path):
    b, st, ln, want = _big_want(ko)
    assert int(want["median"][0]) == case.BIG and int(want["median"][1]) == (1 << 34) + 1 and int(want["median"][2]) == case.BIG
    assert int(want["sum"][0]) == case.BIG + (1 << 34) + 1 + (1 << 32) + 7 and int(want["median"][3]) == case.BIG
    t = engine.table(9, False)
    _, keys, counts = case.big_keys(ko)
    t.merge_host(np.array(keys, np.uint64), np.array(counts, np.uint64))
    _assert_equal(t.record_stats(b, st, ln), want, "LDS select")
    t.free()
    _assert_equal(_in_child("big", 9, False, tmp_path, "big", KATGPU_TEST_STATS_SHORT=0), want, "multi-pass select")
    ones = engine.table(4, False)
    ones.count_bases(np.frombuffer(b"TTTTTTT", np.uint8))               # the all-ones key lives in a scalar counter
    got = ones.record_stats(b"ATTTTTA", [0], [7], False)
    assert tuple(int(got[f][0]) for f in rm.FIELDS) == (8, 4, 2, 0, 0, 0)
    ones.free()


def test_heavy_ties(engine):
    k = 27
    n = 1_200_000                                                        # beyond a packed slot's in-place field: the count is in the side table
    t = engine.table(k, True, size_hint=1 << 23).count_bases(np.frombuffer(b"A" * (n + k - 1), np.uint8))
    assert t.slot_bytes() == 8
    recs = [b"A" * 5000, b"A" * 300, b"A" * 2000 + b"C" + b"A" * 3000, b"A" * k]
    joined, st, ln = rm.join_records(recs)
    got = t.record_stats(joined, st, ln)
    assert [int(x) for x in got["median"]] == [n, n, n, n]
    assert [int(x) for x in got["sum"]] == [n * (5000 - k + 1), n * (300 - k + 1), n * (5001 - k + 1 - k), n]
    assert [int(x) for x in got["non_zero"]] == [5000 - k + 1, 300 - k + 1, 5001 - k + 1 - k, 1]
    assert [int(x) for x in got["invalid"]] == [0, 0, 0, 0] and [int(x) for x in got["gc_bases"]] == [0, 0, 1, 0]
    t.free()


def test_argument_errors(engine):
    t = engine.table(9, True).count_bases(np.frombuffer(b"ACGTACGTTGCATGCA", np.uint8))
    bases = b"ACGTACGTTGCATGCA"
    with pytest.raises(kat_amd.binding.KatGpuError, match="starts before record 0 ends"):
        t.record_stats(bases, [0, 5], [10, 5])
    with pytest.raises(kat_amd.binding.KatGpuError, match="lies beyond the 16 bases"):
        t.record_stats(bases, [0, 10], [5, 7])
    assert t.record_stats(bases, [], []).shape == (0,)
    assert t.record_stats(b"", [0, 0], [0, 0]).tolist() == [(0, 0, 0, 0, 0, 0)] * 2
    t.free()


# ---- the command line: no per-position profile may cross the bus ----

def _run(args, cwd, forbid=True):
    e = dict(os.environ)
    if forbid:
        e["KATGPU_TEST_FORBID_PROFILE_HOST"] = "1"
    return subprocess.run([EXE] + args, cwd=cwd, capture_output=True, text=True, timeout=300, env=e)


def _cli_inputs(refdata, tmp_path):
    """Several thousand records (the reads of the reference's test data and pieces of them, some with N, some shorter than k, one
    empty) and one long contig, as FASTA."""
    from tests import filter_model as fm
    reads = [s for _, s, _ in fm.read_records(os.path.join(refdata, "ecoli_r1.1K.fastq"))]
    recs = []
    for i, s in enumerate(reads):
        recs += [("r%d" % i, s), ("h%d some words" % i, s[: len(s) // 2]), ("n%d" % i, s[:30] + "N" + s[31:70].lower()), ("t%d" % i, s[-(i % 60):] if i % 60 else "")]
    recs.insert(1500, ("contig", "".join(reads[:400]) + "NNNN" + "".join(reads[400:500])))
    fa = tmp_path / "records.fa"
    with open(fa, "w") as f:
        for name, seq in recs:
            f.write(">" + name + "\n" + "".join(seq[i:i + 70] + "\n" for i in range(0, len(seq), 70)))
    assert len(recs) > 4000 and len(recs[1500][1]) > 40000
    return str(fa)


def test_cli_without_profiles(ko, refdata, tmp_path):
    fa = _cli_inputs(refdata, tmp_path)
    r1 = os.path.join(refdata, "ecoli_r1.1K.fastq")
    jf = os.path.join(refdata, "ecoli.header.jf27")
    # kat sect -n, with and without -g; plain input, .jf input, a wide k
    for tag, args, table, kw in (("sp", [fa, r1], lambda: ko.Table(27, True).count_files([r1]), {}),
                                 ("sg", ["-g", "-t", "3", fa, r1], lambda: ko.Table(27, True).count_files([r1]), dict(output_gc_stats=True)),
                                 ("sj", [fa, jf], lambda: ko.Table.from_jf(jf), {}),
                                 ("sw", ["-m", "45", "-g", fa, r1], lambda: ko.WideTable(45, True).count_files([r1]), dict(output_gc_stats=True))):
        r = _run(["sect", "-n", "-H", "1000000", "-o", tag] + args, tmp_path)
        assert r.returncode == 0, r.stderr
        ko.sect(table(), fa, str(tmp_path / ("want_" + tag)), no_count_stats=True, **kw)
        for suffix in ("-stats.tsv",) + (("-counts.gc",) if kw else ()):
            assert (tmp_path / (tag + suffix)).read_bytes() == (tmp_path / ("want_" + tag + suffix)).read_bytes(), (tag, suffix)
        assert not (tmp_path / (tag + "-counts.cvg")).exists()
    # kat cold: reads counted from a file, loaded from a .jf, a wide k
    for tag, args, rd, k in (("cp", [fa, r1], lambda: ko.Table(27, False).count_files([r1]), 27), ("cj", [fa, jf], lambda: ko.Table.from_jf(jf), 27),
                             ("cw", ["-m", "45", fa, r1], lambda: ko.WideTable(45, False).count_files([r1]), 45)):
        r = _run(["cold", "-H", "1000000", "-t", "2", "-o", tag] + args, tmp_path)
        assert r.returncode == 0, r.stderr
        asm = (ko.WideTable(k, False) if k > 32 else ko.Table(k, False)).count_files([fa])
        ko.cold(rd(), asm, fa, str(tmp_path / ("want_" + tag)))
        assert (tmp_path / (tag + "-stats.tsv")).read_bytes() == (tmp_path / ("want_" + tag + "-stats.tsv")).read_bytes(), tag
    # the hook bites: without -n the per-position counts are needed
    r = _run(["sect", "-o", "fails", fa, r1], tmp_path)
    assert r.returncode != 0 and "katgpu_table_profile_host is forbidden" in r.stderr
    assert _run(["sect", "-o", "works", fa, r1], tmp_path, forbid=False).returncode == 0
