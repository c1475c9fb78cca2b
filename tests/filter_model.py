"""Plain-Python restatement of `kat filter kmer` and `kat filter seq` (KAT src/filter_kmer.cc, src/filter_sequence.cc), the yardstick of
tests/test_filter_model.py and tests/test_gpu_filter.py.  Its k-mers come from the oracle (ko.Table(...).dump_sorted()), their GC from
tests/independent.py, its read hits from ko.profile summed per record; its writers follow SeqAn 2.0.0's
(seq_io/fasta_fastq.h:455-505, stream/tokenization.h:464-482)."""
import numpy as np

from tests import independent

# FilterKmer::main / FilterSeq::main defaults (src/filter_kmer.cc:333-346, src/filter_sequence.cc:382-407) -- not the DEFAULT_FILT_*
# constants of the headers (low count 0, high GC 31)
KMER_DEFAULTS = dict(output_prefix="kat.filter.kmer", low_count=1, high_count=10000, low_gc=1, high_gc=100, invert=False, separate=False)
SEQ_DEFAULTS = dict(output_prefix="kat.filter.kmer", threshold=0.1, invert=False, separate=False, frequency=0.0, stats=False)


def route(in_bounds, invert, separate):
    """FilterKmer::filterSlice (src/filter_kmer.cc:262-281): 'keep', 'drop' or None (neither).  With `separate`, invert is ignored."""
    if not separate:
        return "keep" if in_bounds != invert else None
    return "keep" if in_bounds else "drop"


def gc_of(keys, k):
    """#G+#C of packed k-mers; wide k-mers (k > 32) as a (hi, lo) pair of arrays."""
    if k > 32:
        hi, lo = keys
        return independent.gc_count(lo, 32) + independent.gc_count(hi, k - 32)
    return independent.gc_count(keys, k)


def filter_kmer(keys, counts, k, low_count=1, high_count=10000, low_gc=1, high_gc=100, invert=False, separate=False):
    """keys: u64 array (k <= 32) or (hi, lo); counts u64.  Returns (keep mask, drop mask, counters dict) -- the counters of
    FilterKmer::merge (src/filter_kmer.cc:212-230)."""
    c = np.asarray(counts, np.uint64)
    gc = gc_of(keys, k)
    inb = (gc >= low_gc) & (gc <= high_gc) & (c >= np.uint64(low_count)) & (c <= np.uint64(high_count))
    if separate:
        keep, drop = inb, ~inb
    else:
        keep, drop = inb != bool(invert), np.zeros(c.size, bool)
    ctr = dict(all_distinct=int(c.size), all_total=int(c.sum()), keep_distinct=int(keep.sum()), keep_total=int(c[keep].sum()),
               drop_distinct=int(drop.sum()), drop_total=int(c[drop].sum()))
    return keep, drop, ctr


def kmer_stdout_lines(ctr, separate):
    """FilterKmer::merge's lines, byte for byte."""
    lines = ["K-mers in input   : %d distinct; %d total." % (ctr["all_distinct"], ctr["all_total"]),
             "K-mers to keep    : %d distinct; %d total." % (ctr["keep_distinct"], ctr["keep_total"])]
    if separate:
        lines.append("K-mers to discard : %d distinct; %d total." % (ctr["drop_distinct"], ctr["drop_total"]))
    return lines


# ---- filter seq ----

def record_hits(counts, gcs):
    """FilterSeq::getProfile + processSeq's nbFound (src/filter_sequence.cc:333-337, 398-430): windows that are valid and counted."""
    return int(np.count_nonzero((np.asarray(gcs) >= 0) & (np.asarray(counts) > 0)))


def nb_kmers(length, k):
    return max(0, length - k + 1)


def fmt_ratio(hits, nb):
    """`ostream << double` of (double)hits / nb_kmers: %g at precision 6; 0/0 is the x86 default NaN, printed "-nan" by glibc."""
    if nb == 0:
        return "-nan"
    return "%g" % (hits / nb)


def keep_decision(hits, nb, threshold=0.1, invert=False, frequency=0.0, u=0.0):
    """processSeq (src/filter_sequence.cc:339-372).  A record without windows has ratio NaN: both comparisons fail, never kept."""
    if nb == 0:
        return False
    ratio = hits / nb
    if (ratio >= threshold and not invert) or (invert and ratio < threshold):
        return not (0.0 < frequency < u)
    return False


def wrap(s, line):
    """writeWrappedString: lines of `line` characters (0: one line), and always at least one line."""
    if line == 0 or len(s) == 0:
        return s + "\n"
    return "".join(s[i:i + line] + "\n" for i in range(0, len(s), line))


def fasta_record(name, seq):
    return ">" + name + "\n" + wrap(seq, 70)


def fastq_record(name, seq, qual):
    return "@" + name + "\n" + wrap(seq, 0) + "+\n" + wrap(qual, 0)


def read_records(path):
    """(name, seq, qual) of a FASTA (sequence lines joined) or 4-line FASTQ file."""
    return read_records_from_text(open(path).read(), path.endswith((".fq", ".fastq")))


def read_records_from_text(text, fastq):
    out = []
    if fastq:
        lines = text.split("\n")
        for i in range(0, len(lines) - 3, 4):
            if lines[i].startswith("@"):
                out.append((lines[i][1:], lines[i + 1], lines[i + 3]))
        return out
    for block in text.split(">")[1:]:
        head, _, body = block.partition("\n")
        out.append((head, body.replace("\n", ""), ""))
    return out


def filter_seq(recs1, recs2, hits_nb, fastq, threshold=0.1, invert=False, separate=False):
    """The files of `kat filter seq` with -f 0: {"in", "out", "in2", "out2", "stats"} (strings) and keepers / total.
    hits_nb(seq) -> (hits, nb_kmers) of one read; a pair's are added (the hit vectors of R1 and R2 are concatenated)."""
    w = (lambda r: fastq_record(*r)) if fastq else (lambda r: fasta_record(r[0], r[1]))
    paired = recs2 is not None
    o = {"in": [], "out": [], "in2": [], "out2": [], "stats": ["index\tnb_bases\tnb_kmers\tnb_hits\tratio\n"]}
    keepers = 0
    for i, r1 in enumerate(recs1):
        parts = [r1] + ([recs2[i]] if paired else [])
        hits = nb = bases = 0
        for r in parts:
            h, n = hits_nb(r[1])
            hits += h; nb += n; bases += len(r[1])
        keep = keep_decision(hits, nb, threshold, invert)
        if keep:
            keepers += 1
            o["in"].append(w(r1))
            if paired:
                o["in2"].append(w(recs2[i]))
        elif separate:
            o["out"].append(w(r1))
            if paired:
                o["out2"].append(w(recs2[i]))
        o["stats"].append("%d\t%d\t%d\t%d\t%s\n" % (i, bases, nb, hits, fmt_ratio(hits, nb)))
    res = {key: "".join(v) for key, v in o.items()}
    res["keepers"], res["total"] = keepers, len(recs1)
    return res
