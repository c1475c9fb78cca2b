"""The 5' trim through katgpu_count_files' fast paths -- the device record scan (kg_scan.hpp) and the FASTQ host strip (kg_scan.hip:
run_strip) -- against the ORACLE's parser and counter.  kg_scan.hpp states which records are plain under a trim; files of such records
must be parsed by the fast path (scan launches, or the `host strip of` trace line, and no hand-over), files with any other record must be
handed to the host state machine and give the oracle's table or error all the same.

Two halves.  build(dir) -- no GPU -- writes the case files and expected.json: per (file, trim, k, canonical) the oracle's table as
(distinct, total, sha1 of the sorted keys and counts), or its error.  tests/test_gpu_scan_trim.py calls it once per session.  main(), run
by that test in a subprocess under each set of KATGPU_TEST_SCAN_* / KATGPU_TEST_STRIP_* hooks, counts the files on the device and compares."""
import contextlib
import gzip
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kat_amd  # noqa: E402
from kat_amd import synth  # noqa: E402
from oracle import koracle as ko  # noqa: E402
from tests.scan_cases import fasta, fastq  # noqa: E402

TRIMS = (1, 5, 19)
CONFIGS = ((27, True), (27, False), (15, True), (15, False))
PLAIN = ("reads.fq", "plainhdr.fq", "contigs.fa", "wide.fa", "twoline.fa")
DECLINING = ("ragged.fq", "shortfirst.fa", "emptyrec.fa")
GROUP, GROUP_TRIMS = ("reads.fq", "more.fq.gz", "contigs.fa"), (5, 3, 2)
# twoline.fa without a trim as well: a hand-over (KATGPU_TEST_SCAN_FAIL_AT) that begins at a record's '>' must keep the 'N' in front of it
PAIRS = tuple((n, t) for n in PLAIN + DECLINING for t in TRIMS) + (("twoline.fa", 0),)
HANDOVER = ("goes to the host parser", "the host parser takes the file")      # the device scan's line, the strip's


def digest(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(np.ascontiguousarray(a, np.uint64).tobytes())
    return h.hexdigest()


def table_key(table):
    cols = table.dump_sorted()
    return ["ok", int(cols[0].size), int(cols[-1].sum()), digest(*cols)]


def lines(seq, width):
    return b"".join(seq[j:j + width] + b"\n" for j in range(0, len(seq), width))


def build(tmp):
    rng = np.random.default_rng(5)
    g = synth.genome(120000, seed=21)
    reads = [row.tobytes() for row in synth.reads(g, 0, 6000, seed=3).reshape(-1, 151)[:, :150]]
    ragged = [r[: int(rng.integers(1, 151))] for r in reads[:3000]]                    # 1 .. 150 bases: some no longer than any of the trims
    contigs = [g[a:b].tobytes() for a, b in ((0, 50000), (50000, 50007), (50007, 119000), (119000, 120000))]
    two = [g[a:a + int(n)].tobytes() for a, n in zip(rng.integers(0, 119000, 3000), rng.integers(20, 201, 3000))]
    assert min(len(r) for r in ragged) == 1
    cases = {
        "reads.fq": fastq(reads, rng),
        "plainhdr.fq": fastq(reads[:500], rng, qual_at=False, header=lambda i: b"@%d" % i),
        "contigs.fa": fasta(contigs, 60),                                               # the 7-base contig: plain under 1 and 5, not under 19
        "wide.fa": fasta([bytes(rng.choice(np.frombuffer(b"ACGTacgtNn-", np.uint8), size=40000))] * 3, 80),
        "twoline.fa": fasta(two, 10 ** 9),                                              # header, one line of 20 .. 200 bases: half of all line-aligned cuts fall right behind a header
        "ragged.fq": fastq(ragged, rng),
        "shortfirst.fa": fasta(contigs[:2], 60) + b">third\n" + contigs[2][:2] + b"\n" + lines(contigs[2][2:], 60) + fasta(contigs[3:], 60),   # the third record's first line: 2 bases
        "emptyrec.fa": fasta(contigs[:1], 60) + b">nothing here\n" + fasta(contigs[2:], 60),
    }
    for name, data in cases.items():
        with open(os.path.join(tmp, name), "wb") as f:
            f.write(data)
    with gzip.open(os.path.join(tmp, "more.fq.gz"), "wb") as f:
        f.write(fastq(reads[3000:3600], rng))
    expected = {}
    for name, trim in PAIRS:
        path = os.path.join(tmp, name)
        try:
            stream, err = ko.parse_file(path, trim), None
        except ko.OracleError as e:
            stream, err = None, ["err", str(e)]
        for k, canonical in CONFIGS:
            expected["%s/%d/%d/%d" % (name, trim, k, canonical)] = err or table_key(ko.Table(k, canonical).count_bases(stream))
    for name in ("reads.fq", "contigs.fa"):
        expected["%s/5/45/1" % name] = table_key(ko.WideTable(45, True).count_bases(ko.parse_file(os.path.join(tmp, name), 5)))
    expected["group"] = table_key(ko.Table(27, True).count_files([os.path.join(tmp, n) for n in GROUP], list(GROUP_TRIMS)))
    # what the rule of kg_scan.hpp says about these files, so that the oracle's verdicts are the ones the cases were built for
    assert all(expected["%s/%d/27/1" % (n, t)][0] == "ok" for n in PLAIN for t in TRIMS)
    assert all(expected["ragged.fq/%d/27/1" % t] == ["err", "Invalid fastq sequence"] for t in TRIMS)
    with open(os.path.join(tmp, "expected.json"), "w") as f:
        json.dump(expected, f)


def declines(name, trim):
    """Must the fast path hand this file over (a record that is not plain under the trim)?"""
    if name == "shortfirst.fa":
        return trim >= 2                                            # its 2-base first line (and, from 7 on, the 7-base contig)
    return name in DECLINING or (name == "contigs.fa" and trim >= 7)


@contextlib.contextmanager
def trace():
    """The library's KATGPU_TRACE lines (stderr of this process) while the block runs: box[0] afterwards."""
    box = [""]
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            yield box
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            f.seek(0)
            box[0] = f.read().decode(errors="replace")
            sys.stderr.write(box[0])


def count(eng, k, canonical, paths, trims):
    """(table key or error, trace text, scan launches) of one katgpu_count_files call."""
    eng.profile_reset()
    t = eng.table(k, canonical, size_hint=1 << 18)
    with trace() as box:
        try:
            t.count_files(paths, trims)
            got = table_key(t)
        except kat_amd.KatGpuError as e:
            assert e.code == 4, e
            got = ["err", e.message]
    t.free()
    return got, box[0], eng.profile()["scan"]["launches"]


def main():
    tmp = sys.argv[1]
    with open(os.path.join(tmp, "expected.json")) as f:
        expected = json.load(f)
    scan_fail, strip_fail = "KATGPU_TEST_SCAN_FAIL_AT" in os.environ, "KATGPU_TEST_STRIP_FAIL_AT" in os.environ      # hook sets that hand plain files over too
    forced = scan_fail or strip_fail
    strip_hook = bool(os.environ.get("KATGPU_TEST_STRIP_SEGMENT"))
    eng = kat_amd.Engine(0)
    n = 0
    for name, trim in PAIRS:
        path = os.path.join(tmp, name)
        stripped = name.endswith(".fq") and strip_hook
        for k, canonical in CONFIGS:
            got, err, launches = count(eng, k, canonical, [path], [trim])
            what = (name, trim, k, canonical)
            assert got == expected["%s/%d/%d/%d" % (name, trim, k, int(canonical))], (what, got, err[-600:])
            handed = any(h in err for h in HANDOVER)
            if declines(name, trim):
                assert handed, (what, "no hand-over to the host parser", err[-600:])
            else:
                if stripped:
                    assert launches == 0 and "host strip of" in err, (what, launches, err[-600:])
                else:
                    assert launches > 0, (what, "the device scan did not run")
                assert handed == (strip_fail if stripped else scan_fail), (what, err[-600:])
            n += 1
    for name in ("reads.fq", "contigs.fa"):                         # k > 32: the trimmed stream goes to the wide counter
        got, err, launches = count(eng, 45, True, [os.path.join(tmp, name)], [5])
        assert got == expected["%s/5/45/1" % name], (name, "k = 45", got)
        assert launches > 0 or (name.endswith(".fq") and strip_hook and "host strip of" in err), (name, "k = 45: no fast path")
        n += 1
    got, err, launches = count(eng, 27, True, [os.path.join(tmp, g) for g in GROUP], list(GROUP_TRIMS))       # scanned, streamed, scanned
    assert got == expected["group"], ("group", got)
    assert launches > 0 and (forced or not any(h in err for h in HANDOVER)), ("group", launches, err[-600:])
    n += 1
    if not forced:
        # two ranks' shares of one trimmed FASTQ file, merged on the host
        keys, counts = [], []
        for r in (0, 1):
            t = eng.table(27, True, size_hint=1 << 18)
            t.count_files_sharded([os.path.join(tmp, "reads.fq")], r, 2, [5])
            kk, cc = t.export()
            keys.append(kk[cc > 0]); counts.append(cc[cc > 0])
            t.free()
        uk, inv = np.unique(np.concatenate(keys), return_inverse=True)
        uc = np.zeros(uk.size, np.uint64)
        np.add.at(uc, inv, np.concatenate(counts))
        assert ["ok", int(uk.size), int(uc.sum()), digest(uk, uc)] == expected["reads.fq/5/27/1"], "sharded"
        # a file the ranks cannot share under this trim: still an error, and it says why
        t = eng.table(27, True, size_hint=1 << 18)
        try:
            t.count_files_sharded([os.path.join(tmp, "ragged.fq")], 0, 2, [5])
            raise AssertionError("ragged.fq between two ranks under a trim of 5: no error")
        except kat_amd.KatGpuError as e:
            assert e.code == 4 and "5' trim" in e.message and "run it on one" in e.message, e.message
        t.free()
        n += 2
    print("scan trim cases ok:", n)


if __name__ == "__main__":
    main()
