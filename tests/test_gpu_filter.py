"""`kat filter` on the device: katgpu_table_filter and katgpu_table_seq_hits_* against tests/filter_model.py, and `katgpu filter kmer|seq`
end to end (files byte for byte, stdout lines, errors)."""
import gzip
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from kat_amd import synth
from tests import filter_model as fm
from tests import host_batch_case as hb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kat_amd", "bin", "katgpu")


def run(args, cwd):
    return subprocess.run([EXE] + args, cwd=cwd, capture_output=True, text=True, timeout=300)


def _bases(seed, n_genome=60000, poly=0, t_run=0):
    """Random genome reads with N, lowercase, a poly-A run of `poly` bases (its k-mer's count beyond a packed slot's field) and a T run."""
    rng = np.random.default_rng(seed)
    g = synth.genome(n_genome, seed=seed)
    parts = [g.tobytes(), b"N", synth.reads(g, 0, 300, seed=seed + 1)[:20000].tobytes().lower(), b"\n"]
    if poly:
        parts += [b"A" * poly, b"\n"]
    if t_run:
        parts += [b"T" * t_run, b"\n"]
    parts.append(bytes(rng.choice(list(b"ACGTN"), 3000)))
    return b"".join(parts)


BOXES = [dict(), dict(low_count=2, high_count=40, low_gc=3, high_gc=12), dict(low_count=1, high_count=1, low_gc=0, high_gc=100),
         dict(low_count=100, high_count=10 ** 9, low_gc=0, high_gc=100)]
CASES = [  # k, canonical, size hint (0: the default), poly-A bases, T run
    (5, True, 0, 0, 0), (17, True, 1 << 20, 0, 0), (27, True, 1 << 23, 600000, 0), (31, True, 0, 0, 0),
    (32, True, 0, 0, 0), (32, False, 0, 0, 200), (51, True, 0, 0, 0)]


def _dump(t, k):
    if k > 32:
        hi, lo, c = t.dump_sorted()
        return (hi, lo), c
    return t.dump_sorted()


def _eq_keys(a, b, k):
    if k > 32:
        return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    return np.array_equal(a, b)


def _sel(keys, m, k):
    return (keys[0][m], keys[1][m]) if k > 32 else keys[m]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "k%d%s%s" % (c[0], "" if c[1] else "N", "-ovf" if c[3] else ""))
def test_filter_abi_against_model(engine, ko, case):
    k, canon, hint, poly, trun = case
    b = _bases(k * 7 + 1, poly=poly, t_run=trun)
    t = engine.table(k, canon, size_hint=hint).count_bases(b)
    o = (ko.WideTable(k, canon) if k > 32 else ko.Table(k, canon)).count_bases(b)
    keys, counts = _dump(o, k)
    if k <= 32:
        gk, gc_ = t.dump_sorted()
        assert np.array_equal(gk, keys) and np.array_equal(gc_, counts)
    if poly:
        assert t.slot_bytes() == 8 and counts.max() > (1 << 19)               # a packed table whose side table holds the poly-A count
    if trun:
        assert keys[-1] == np.uint64(2 ** 64 - 1)                           # the all-T k-mer (the empty marker's value) is present
    hin = t.hist()
    for box in BOXES:
        for invert in (False, True):
            for separate in (False, True):
                keep, drop, ctr = t.filter(invert=invert, separate=separate, **{**dict(low_count=1, high_count=10000, low_gc=1, high_gc=100), **box})
                mk, md, mctr = fm.filter_kmer(keys, counts, k, invert=invert, separate=separate,
                                              **{**dict(low_count=1, high_count=10000, low_gc=1, high_gc=100), **box})
                what = (box, invert, separate)
                assert ctr == mctr, what
                kk, kc = _dump(keep, k)
                assert _eq_keys(kk, _sel(keys, mk, k), k) and np.array_equal(kc, counts[mk]), what
                st = keep.stats()
                assert st["distinct"] == mctr["keep_distinct"] and st["total"] == mctr["keep_total"], what
                hk = keep.hist()
                # lookups on the kept table: every kept count, 0 for every other key (the probe chains are intact)
                got = keep.get_wide(keys[0], keys[1]) if k > 32 else keep.get(keys)
                assert np.array_equal(got, np.where(mk, counts, 0)), what
                if separate:
                    dk, dc = _dump(drop, k)
                    assert _eq_keys(dk, _sel(keys, md, k), k) and np.array_equal(dc, counts[md]), what
                    assert mctr["keep_distinct"] + mctr["drop_distinct"] == mctr["all_distinct"]
                    assert np.array_equal(hk + drop.hist(), hin), what
                    got = drop.get_wide(keys[0], keys[1]) if k > 32 else drop.get(keys)
                    assert np.array_equal(got, np.where(md, counts, 0)), what
                    drop.free()
                else:
                    assert drop is None
                keep.free()
    # the input is left as it was
    k2, c2 = _dump(t, k)
    assert _eq_keys(k2, keys, k) and np.array_equal(c2, counts)


def _records(rng, k):
    """Reads with N and lowercase, lengths 0, k-1, k, records crossing a kernel chunk (4064 window starts), runs of empty records."""
    g = synth.genome(30000, seed=11).tobytes().decode()
    recs = []
    for L in [0, k - 1, k, k + 1, 0, 0, 5000, 9000, 150, 151, 0]:
        s0 = int(rng.integers(0, len(g) - L)) if L else 0
        recs.append(g[s0:s0 + L])
    for _ in range(400):
        L = int(rng.integers(0, 300))
        s0 = int(rng.integers(0, len(g) - L))
        s = list(g[s0:s0 + L])
        for _ in range(int(rng.integers(0, 3))):
            if s:
                s[int(rng.integers(0, len(s)))] = "N"
        if rng.random() < 0.3:
            s = [c.lower() for c in s]
        if rng.random() < 0.2:
            s = list("".join(rng.choice(list("ACGT"), len(s))))
        recs.append("".join(s))
    recs += [""] * 3000 + ["ACGT" * 40]                                     # more records in one chunk than the kernel's LDS bins
    return recs


@pytest.mark.parametrize("k,canon", [(17, True), (27, False), (31, True), (51, True)])
def test_seq_hits_against_profile(engine, ko, k, canon):
    rng = np.random.default_rng(k)
    b = synth.reads(synth.genome(30000, seed=11), 0, 600, seed=5)
    t = engine.table(k, canon).count_bases(b)
    o = (ko.WideTable(k, canon) if k > 32 else ko.Table(k, canon)).count_bases(b)
    recs = _records(rng, k)
    starts = np.cumsum([0] + [len(s) for s in recs[:-1]]).astype(np.uint64)
    lens = np.array([len(s) for s in recs], np.uint64)
    joined = "".join(recs).encode()
    for canonicalise in (False, True):
        want = np.array([fm.record_hits(*ko.profile(o, s, canonicalise)) if s else 0 for s in recs], np.uint64)
        assert want.sum() > 0
        got = t.seq_hits(joined, starts, lens, canonicalise)
        assert np.array_equal(got, want), (k, canonicalise, np.nonzero(got != want)[0][:10])
        # device form, bases at an odd address, records with gaps between them (a separator byte before every record)
        sep = b"".join(b"N" + s.encode() for s in recs)
        st2 = starts + np.arange(1, len(recs) + 1, dtype=np.uint64)
        db = engine.alloc(len(sep) + 17)
        db.upload(np.frombuffer(sep, np.uint8), offset=1)
        dr = engine.alloc(3 * 8 * len(recs))
        dr.upload(st2)
        dr.upload(lens, offset=8 * len(recs))
        t.seq_hits_device(db.ptr + 1, len(sep), dr.ptr, dr.ptr + 8 * len(recs), len(recs), dr.ptr + 16 * len(recs), canonicalise)
        engine.sync()
        assert np.array_equal(dr.download(np.uint64, len(recs), offset=16 * len(recs)), want)
        db.free(); dr.free()


@pytest.mark.parametrize("k,canon", [(27, False), (51, True)])
def test_seq_hits_host_in_many_batches(ko, tmp_path, k, canon):
    """katgpu_table_seq_hits_host with batches of 4000 bases: the records of 5000 and 9000 bases are batches of their own, the run of 3000
    empty records spans cuts, and every record's hits equal what one batch gives (the model's count over the oracle's profile)."""
    o = (ko.WideTable(k, canon) if k > 32 else ko.Table(k, canon)).count_bases(hb.counted())
    b, st, ln, recs = hb.hits_records(k)
    assert int(ln.max()) == 9000 and int((ln == 0).sum()) >= 3000 and b"".join(s.encode() for s in recs) == b
    for canonicalise in (False, True):
        want = np.array([fm.record_hits(*ko.profile(o, s, canonicalise)) if s else 0 for s in recs], np.uint64)
        assert want.sum() > 0
        out = str(tmp_path / ("hits%d.npy" % canonicalise))
        r = subprocess.run([sys.executable, "-m", "tests.host_batch_case", "hits", str(k), str(int(canon)), str(int(canonicalise)), "0", out], cwd=ROOT,
                           env={**os.environ, "KATGPU_TEST_HITS_BATCH": "4000"}, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert len(b) > 60000 and int(open(out + ".sections").read()) > 10              # the hook bites: but for the two long records', no batch holds more than 4000 bases
        got = np.load(out)
        assert got.dtype == np.uint64 and np.array_equal(got, want), (k, canonicalise, np.nonzero(got != want)[0][:10])


# ---- the command line ----

def _jf_dump(ko, path, k):
    t = ko.Table.from_jf(path) if k <= 32 else None
    return t.dump_sorted()


def test_filter_kmer_cli(ko, refdata, tmp_path):
    r1 = os.path.join(refdata, "ecoli_r1.1K.fastq")
    o = ko.Table(27, True).count_files([r1])
    keys, counts = o.dump_sorted()
    for args, box, sep, inv in [([], {}, False, False), (["-c", "2", "-d", "30", "-g", "5", "-h", "15", "-s"], dict(low_count=2, high_count=30, low_gc=5, high_gc=15), True, False),
                                (["-c", "2", "-i"], dict(low_count=2), False, True)]:
        (tmp_path / "f-in.jf27").write_bytes(b"stale")                      # an existing target is replaced
        r = run(["filter", "kmer", "-o", "f"] + args + [r1], tmp_path)
        assert r.returncode == 0, r.stderr
        mk, md, ctr = fm.filter_kmer(keys, counts, 27, separate=sep, invert=inv, **box)
        lines = r.stdout.splitlines()
        for want in fm.kmer_stdout_lines(ctr, sep):
            assert want in lines, (want, r.stdout)
        assert ("K-mers to discard" in r.stdout) == sep
        gk, gc_ = _jf_dump(ko, str(tmp_path / "f-in.jf27"), 27)
        assert np.array_equal(gk, keys[mk]) and np.array_equal(gc_, counts[mk])
        if sep:
            gk, gc_ = _jf_dump(ko, str(tmp_path / "f-out.jf27"), 27)
            assert np.array_equal(gk, keys[md]) and np.array_equal(gc_, counts[md])
        for f in ("f-in.jf27", "f-out.jf27"):
            if (tmp_path / f).exists():
                os.unlink(tmp_path / f)
    # LOAD mode, default output prefix
    jf = os.path.join(refdata, "ecoli.header.jf27")
    r = run(["filter", "kmer", "-c", "3", jf], tmp_path)
    assert r.returncode == 0, r.stderr
    src = ko.Table.from_jf(jf)
    keys, counts = src.dump_sorted()
    mk, _, ctr = fm.filter_kmer(keys, counts, 27, low_count=3)
    assert fm.kmer_stdout_lines(ctr, False)[0] in r.stdout.splitlines()
    gk, gc_ = _jf_dump(ko, str(tmp_path / "kat.filter.kmer-in.jf27"), 27)
    assert np.array_equal(gk, keys[mk]) and np.array_equal(gc_, counts[mk])
    r = run(["filter", "kmer", "-c", "5", "-d", "4", jf], tmp_path)
    assert r.returncode == 4 and "High kmer count value must be >= to low kmer count value" in r.stderr


def _write_fasta(path, recs):
    with open(path, "w") as f:
        for name, seq, _ in recs:
            f.write(">" + name + "\n" + "".join(seq[i:i + 60] + "\n" for i in range(0, len(seq), 60)))


def _hits_nb(ko, table, k):
    return lambda s: (fm.record_hits(*ko.profile(table, s)) if len(s) >= k else 0, fm.nb_kmers(len(s), k))


def _check_seq_outputs(tmp_path, prefix, res, ext, paired, separate, stats):
    r1 = ".R1" if paired else ""
    assert (tmp_path / (prefix + ".in" + r1 + ext)).read_text() == res["in"]
    if paired:
        assert (tmp_path / (prefix + ".in.R2" + ext)).read_text() == res["in2"]
    assert (tmp_path / (prefix + ".out" + r1 + ext)).exists() == separate
    if separate:
        assert (tmp_path / (prefix + ".out" + r1 + ext)).read_text() == res["out"]
        if paired:
            assert (tmp_path / (prefix + ".out.R2" + ext)).read_text() == res["out2"]
    if stats:
        assert (tmp_path / (prefix + ".stats")).read_text() == res["stats"]


def test_filter_seq_cli(ko, refdata, tmp_path):
    fq1, fq2 = os.path.join(refdata, "ecoli_r1.1K.fastq"), os.path.join(refdata, "ecoli_r2.1K.fastq")
    hash_src = os.path.join(refdata, "ecoli_r1.1K.fastq")
    o = ko.Table(27, True).count_files([hash_src])
    hn = _hits_nb(ko, o, 27)
    q1, q2 = fm.read_records(fq1), fm.read_records(fq2)
    # FASTA input: reads of the other file, some records empty / shorter than k / with N
    fa_recs = [(n, s, "") for n, s, _ in q2[:300]] + [("empty", "", ""), ("short", "ACGT", ""), ("withN", q1[0][1][:40] + "N" + q1[0][1][40:], "")]
    fa = tmp_path / "reads.fa"
    _write_fasta(fa, fa_recs)
    for args, kw in [([], {}), (["-T", "0.5", "-s", "--stats"], dict(threshold=0.5, separate=True)),
                     (["-i", "-s", "--stats"], dict(invert=True, separate=True)), (["-T", "0.0", "--stats"], dict(threshold=0.0))]:
        r = run(["filter", "seq", "-o", "fs", "--seq", str(fa)] + args + [hash_src], tmp_path)
        assert r.returncode == 0, r.stderr
        res = fm.filter_seq(fa_recs, None, hn, False, **kw)
        _check_seq_outputs(tmp_path, "fs", res, ".fa", False, kw.get("separate", False), "--stats" in args)
        assert "Found %d / %d to keep" % (res["keepers"], res["total"]) in r.stdout.splitlines()
        for f in os.listdir(tmp_path):
            if f.startswith("fs."):
                os.unlink(tmp_path / f)
    # FASTQ, single and paired
    for args, kw, paired in [(["-s", "--stats"], dict(separate=True), False), (["-T", "0.3", "-s", "--stats", "--seq2", fq2], dict(threshold=0.3, separate=True), True),
                             (["-i", "--seq2", fq2], dict(invert=True), True)]:
        r = run(["filter", "seq", "-o", "fq", "--seq", fq1] + args + [hash_src], tmp_path)
        assert r.returncode == 0, r.stderr
        res = fm.filter_seq(q1, q2 if paired else None, hn, True, **kw)
        _check_seq_outputs(tmp_path, "fq", res, ".fastq", paired, kw.get("separate", False), "--stats" in args)
        assert "Found %d / %d to keep" % (res["keepers"], res["total"]) in r.stdout.splitlines()
        for f in os.listdir(tmp_path):
            if f.startswith("fq."):
                os.unlink(tmp_path / f)
    # -f 0.5 -s: every record in exactly one of in / out, in input order; the kept ones a subset of the -f 0 set
    r = run(["filter", "seq", "-o", "sub", "--seq", fq1, "-f", "0.5", "-s", hash_src], tmp_path)
    assert r.returncode == 0, r.stderr
    full = fm.filter_seq(q1, None, hn, True)
    got_in, got_out = fm.read_records(str(tmp_path / "sub.in.fastq")), fm.read_records(str(tmp_path / "sub.out.fastq"))
    assert len(got_in) + len(got_out) == len(q1)
    names_in = [x[0] for x in got_in]
    order = {x[0]: i for i, x in enumerate(q1)}
    assert [order[n] for n in names_in] == sorted(order[n] for n in names_in)
    assert [order[x[0]] for x in got_out] == sorted(order[x[0]] for x in got_out)
    assert set(names_in) <= {x[0] for x in fm.read_records_from_text(full["in"], True)}
    assert sorted(names_in + [x[0] for x in got_out]) == sorted(x[0] for x in q1)
    # errors: a longer R2; an extension SeqAn cannot write (.gz: the output is <prefix>.in.gz)
    short = tmp_path / "short_r1.fastq"
    short.write_text("".join(fm.fastq_record(*x) for x in q1[:10]))
    r = run(["filter", "seq", "-o", "e", "--seq", str(short), "--seq2", fq2, hash_src], tmp_path)
    assert r.returncode == 4 and "Second sequence file appears to be longer than the first." in r.stderr
    gz = tmp_path / "reads.fastq.gz"
    gz.write_bytes(gzip.compress(open(fq1, "rb").read()))
    r = run(["filter", "seq", "-o", "g", "--seq", str(gz), hash_src], tmp_path)
    assert r.returncode == 5 and "Error: Unknown file extension of g.in.gz: iostream error" in r.stderr


def test_filter_workflow(ko, refdata, tmp_path):
    """count reads -> filter kmer on a count band -> .jf -> filter seq against that .jf, as the model does it."""
    fq1, fq2 = os.path.join(refdata, "ecoli_r1.1K.fastq"), os.path.join(refdata, "ecoli_r2.1K.fastq")
    r = run(["filter", "kmer", "-o", "band", "-c", "2", "-d", "20", fq1, fq2], tmp_path)
    assert r.returncode == 0, r.stderr
    o = ko.Table(27, True).count_files([fq1, fq2])
    keys, counts = o.dump_sorted()
    mk, _, _ = fm.filter_kmer(keys, counts, 27, low_count=2, high_count=20)
    band = ko.Table.from_jf(str(tmp_path / "band-in.jf27"))
    bk, bc = band.dump_sorted()
    assert np.array_equal(bk, keys[mk]) and np.array_equal(bc, counts[mk])
    r = run(["filter", "seq", "-o", "wf", "-T", "0.2", "-s", "--stats", "--seq", fq1, "--seq2", fq2, "band-in.jf27"], tmp_path)
    assert r.returncode == 0, r.stderr
    res = fm.filter_seq(fm.read_records(fq1), fm.read_records(fq2), _hits_nb(ko, band, 27), True, threshold=0.2, separate=True)
    _check_seq_outputs(tmp_path, "wf", res, ".fastq", True, True, True)
    assert 0 < res["keepers"] < res["total"]


def test_filter_at_size(engine):
    """A table of 2^28 slots from synthetic reads: hist(keep) + hist(drop) = hist(input) and the counters against sums of hist bins."""
    t0 = time.time()
    k = 27
    g = engine.synth_genome(20_000_000, 3)
    n_reads = 600_000
    reads = engine.synth_reads(g, 20_000_000, 0, n_reads, seed=4)
    t = engine.table(k, True, size_hint=1 << 28)
    t.count_bases_device(reads.ptr, n_reads * 151)
    hin = t.hist(1, 10000)
    keep, drop, ctr = t.filter(low_count=2, high_count=30, low_gc=0, high_gc=100, separate=True)
    hk, hd = keep.hist(1, 10000), drop.hist(1, 10000)
    assert np.array_equal(hk + hd, hin)
    st = t.stats()
    assert ctr["all_distinct"] == st["distinct"] == int(hin.sum()) and ctr["all_total"] == st["total"]
    # GC 0..100 lets everything through the GC side: the kept set is exactly the count band's bins (labels 1 .. 10001, the last a catch-all)
    assert ctr["keep_distinct"] == int(hin[1:30].sum()) == int(hk.sum()) and ctr["drop_distinct"] == int(hd.sum())
    assert ctr["keep_total"] == int((hin[1:30] * np.arange(2, 31, dtype=np.uint64)).sum())
    assert ctr["keep_total"] + ctr["drop_total"] == ctr["all_total"]
    keep.free(); drop.free(); t.free(); reads.free(); g.free()
    assert time.time() - t0 < 240
