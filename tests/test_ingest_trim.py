"""The 5' trim on the host's fast ingest paths (no GPU needed): the thread team (kg_ingest.cpp: parse_file_parallel) and the FASTQ strip
(strip_fastq_records, C ABI katgpu_strip_fastq_trim) against the oracle's parser.  kg_scan.hpp states which records are plain under a
trim; everything else -- a first sequence line no longer than the trim, a stop byte right behind it, a header behind a header -- must
come out as the streaming machine (and the oracle) say, by way of the hand-over."""
import numpy as np
import pytest

import kat_amd
from kat_amd import binding

TEAM = {"KATGPU_INGEST_MIN_BYTES": "0", "KATGPU_INGEST_MARGIN": "4096", "KATGPU_INGEST_THREADS": "5", "KATGPU_TRACE": "1"}


def _env(monkeypatch, **kw):
    for k, v in kw.items():
        monkeypatch.setenv(k, str(v))


def _clean_records():
    rng = np.random.default_rng(5)                      # the records of test_ingest_parser's team test
    return ["".join(rng.choice(list("ACGTN"), int(rng.integers(30, 200)))) for _ in range(400)]


def _oracle(ko, path, trim):
    """('ok', stream) or ('err', message) as the oracle's parser has it."""
    try:
        return "ok", ko.parse_file(str(path), trim).tobytes()
    except ko.OracleError as e:
        return "err", str(e)


def _library(path, trim):
    try:
        return "ok", kat_amd.parse_file(str(path), trim).tobytes()
    except kat_amd.KatGpuError as e:
        assert e.code == 4                               # KATGPU_ERR_FASTQ, the oracle's code 3
        return "err", e.message


@pytest.mark.parametrize("seg", [1000, 37])
@pytest.mark.parametrize("trim", [1, 7, 29])
def test_team_takes_clean_files_under_a_trim(ko, tmp_path, monkeypatch, capfd, seg, trim):
    recs = _clean_records()
    fa, fq = tmp_path / "clean.fa", tmp_path / "clean.fq"
    fa.write_text("".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(recs)))
    fq.write_text("".join("@r%d\n%s\n+\n%s\n" % (i, r, "@" * len(r)) for i, r in enumerate(recs)))
    want = "N".join(r[trim:] for r in recs).encode()
    for p in (fa, fq):
        assert ko.parse_file(str(p), trim).tobytes() == want
        _env(monkeypatch, KATGPU_INGEST_MIN_BYTES=1 << 60)
        streamed = kat_amd.parse_file(str(p), trim).tobytes()
        _env(monkeypatch, KATGPU_INGEST_SEGMENT=seg, **TEAM)
        capfd.readouterr()
        got = kat_amd.parse_file(str(p), trim).tobytes()
        err = capfd.readouterr().err
        assert got == want and got == streamed, p
        assert "all accepted" in err and "streaming from offset" not in err, err


TRAPS = {          # at trim 3; the streams in the comments are the oracle's
    "short.fa": b">a\nAC\nGGGGTTTT\n>b\nTTGGCCAA\n",                     # GGGGTTTTNGCCAA: the trim eats 'A', 'C', '\n'
    "exact.fa": b">a\nACG\nGGGGTTTT\n>b\nTTGGCCAA\n",                    # GGGGTTTTNGCCAA
    "hdrhdr.fa": b">a\n>b\nTTGGCCAA\nACGT\n>c\nAAAACCCC\n",              # TTGGCCAAACGTNACCCC: the trim eats '>b\n'
    "stop.fa": b">a\nACG>TTT\nGGGG\n>b\nTTGGCCAA\n",                     # NGNGCCAA: '>TTT' becomes a header
    "lasthdr.fa": b">a\nACGTACGT\n>b\n",                                 # TACGTN
    "short.fq": b"@a\nACGTACGT\n+\nIIIIIIII\n@b\nAC\n+\nII\n@c\nTTGGCCAA\n+\nIIIIIIII\n",
    "exact.fq": b"@a\nACGTACGT\n+\nIIIIIIII\n@b\nACG\n+\nIII\n@c\nTTGGCCAA\n+\nIIIIIIII\n",
    "plus.fq": b"@a\nACGTACGT\n+\nIIIIIIII\n@b\nACG+ACGT\n+\nIIIIIIII\n@c\nTTGGCCAA\n+\nIIIIIIII\n",
}
TRAP_STREAMS = {"short.fa": b"GGGGTTTTNGCCAA", "exact.fa": b"GGGGTTTTNGCCAA", "hdrhdr.fa": b"TTGGCCAAACGTNACCCC", "stop.fa": b"NGNGCCAA", "lasthdr.fa": b"TACGTN"}


def _short_every_tenth(fastq):
    rng = np.random.default_rng(9)
    recs = ["".join(rng.choice(list("ACGT"), int(rng.integers(1, 4)) if i % 10 == 9 else int(rng.integers(30, 200)))) for i in range(400)]
    if fastq:
        return "".join("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)) for i, r in enumerate(recs)).encode()
    return "".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(recs)).encode()


@pytest.mark.parametrize("seg", [1000, 37])
def test_team_hands_trapped_records_to_the_machine(ko, tmp_path, monkeypatch, capfd, seg):
    cases = dict(TRAPS)
    cases["tenth.fa"] = _short_every_tenth(False)
    cases["tenth.fq"] = _short_every_tenth(True)
    for name, data in cases.items():
        p = tmp_path / name
        p.write_bytes(data)
        want = _oracle(ko, p, 3)
        if name in TRAP_STREAMS:
            assert want == ("ok", TRAP_STREAMS[name]), name
        if name.endswith(".fq"):
            assert want == ("err", "Invalid fastq sequence"), name
        _env(monkeypatch, KATGPU_INGEST_MIN_BYTES=1 << 60)
        assert _library(p, 3) == want, (name, "streaming")
        _env(monkeypatch, KATGPU_INGEST_SEGMENT=seg, **TEAM)
        capfd.readouterr()
        assert _library(p, 3) == want, (name, "team")
        err = capfd.readouterr().err
        if name == "tenth.fa" and seg == 37:              # every record start is a guessed cut here (the records are longer than a segment): the one
            assert "streaming from offset" in err, err    # behind the first three-symbol record finds the machine reading a '>' line as sequence


def _fq(reads):
    return b"".join(b"@r%d x\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads))


def test_strip_under_a_trim(ko, tmp_path):
    rng = np.random.default_rng(3)
    reads = [bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=int(rng.integers(9, 160)))) for _ in range(300)]
    data = _fq(reads)
    p = tmp_path / "plain.fq"
    p.write_bytes(data)
    for t in (0, 1, 7):
        got = kat_amd.strip_fastq(data, t)
        assert got is not None and got[:-1] == ko.parse_file(str(p), t).tobytes(), t      # (the strip ends every record with 'N', the last one too)
        assert got == b"".join(r[t:] + b"N" for r in reads)
    assert kat_amd.strip_fastq(data, 0) == kat_amd.strip_fastq(data) == binding.strip_fastq(data)
    good = [b"ACGTACGTACGT", b"TTGGCCAATTGG"]
    for t in (1, 3, 7):
        declined = binding.strip_fastq(_fq([good[0], b"", good[1]]))     # what the untrimmed strip says to a record it does not take
        assert declined is None
        for what, read in (("length t", b"ACGTACGT"[:t]), ("length t - 1", b"ACGTACGT"[:t - 1]), ("'+' at byte t", b"ACGTACGT"[:t] + b"+ACG")):
            assert kat_amd.strip_fastq(_fq([good[0], read, good[1]]), t) is declined, (t, what)
        assert kat_amd.strip_fastq(_fq([good[0], b"ACGTACGT"[:t] + b"A", good[1]]), t) == good[0][t:] + b"NAN" + good[1][t:] + b"N"
        assert kat_amd.strip_fastq(_fq([good[0], b"+" * t + b"ACG", good[1]]), t) == good[0][t:] + b"NACGN" + good[1][t:] + b"N"    # a '+' the trim drops
