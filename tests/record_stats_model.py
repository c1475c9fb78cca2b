"""katgpu_table_record_stats_* restated in numpy: the six per-record fields from the bases, the records, k and the per-position
counts (oracle.koracle.profile over the same bases), and the -stats.tsv rows `katgpu sect` / `katgpu cold` print from them
(Sect::processSeq + printStatTable, src/sect.cc:490-589,427-445; Cold::processSeq + printStatTable, src/cold.cc:303-406,254-271)."""
import numpy as np

FIELDS = ("sum", "median", "non_zero", "invalid", "gc_bases", "n_bases")
DTYPE = np.dtype([(f, np.uint64) for f in FIELDS])

_IS_BASE = np.zeros(256, bool)
_IS_BASE[list(b"ACGTacgt")] = True
_IS_GC = np.zeros(256, bool)
_IS_GC[list(b"GgCc")] = True
_IS_N = np.zeros(256, bool)
_IS_N[list(b"Nn")] = True

SECT_HEADER = b"seq_name\tmedian\tmean\tgc%\tseq_length\tkmers_in_seq\tinvalid_kmers\t%_invalid\tnon_zero_kmers\t%_non_zero\t%_non_zero_corrected\n"
COLD_HEADER = b"seq_name\tread_median_cvg\tread_mean_cvg\tasm_cn\tgc%\tseq_length\tkmers_in_seq\tinvalid_kmers\t%_invalid\tnon_zero_kmers\t%_non_zero\t%_non_zero_corrected\n"


def as_bytes(bases):
    if isinstance(bases, str):
        bases = bases.encode()
    return np.frombuffer(bases, np.uint8) if isinstance(bases, (bytes, bytearray)) else np.ascontiguousarray(bases, np.uint8)


def one_record(seq, counts, k):
    """seq: the record's bytes (u8); counts: the count of each of its len - k + 1 windows (ignored where the window is invalid)."""
    out = np.zeros((), DTYPE)
    n = seq.size
    out["gc_bases"] = int(_IS_GC[seq].sum())
    out["n_bases"] = int(_IS_N[seq].sum())
    nb = n - k + 1 if n >= k else 0
    if nb:
        bad = np.concatenate([[0], np.cumsum(~_IS_BASE[seq])])
        invalid = (bad[k:] - bad[:-k]) > 0
        c = np.where(invalid, np.uint64(0), np.asarray(counts[:nb], np.uint64))
        out["invalid"] = int(invalid.sum())
        v = c[~invalid]                                         # exact for any counts: the two halves are summed apart
        out["sum"] = ((int((v >> np.uint64(32)).sum()) << 32) + int((v & np.uint64(0xFFFFFFFF)).sum())) & (2 ** 64 - 1)
        out["non_zero"] = int((c[~invalid] != 0).sum())
        out["median"] = np.sort(c)[nb // 2]
    return out


def record_stats(bases, rec_start, rec_len, k, counts):
    """counts[i] = the count of the window starting at bases[i] (koracle.profile of the whole buffer, or any array that is right on
    the windows inside records)."""
    b = as_bytes(bases)
    out = np.zeros(len(rec_start), DTYPE)
    for r, (s, n) in enumerate(zip(rec_start, rec_len)):
        s, n = int(s), int(n)
        out[r] = one_record(b[s:s + n], counts[s:s + max(0, n - k + 1)], k)
    return out


def _u32_of_double(x):
    return int(float(int(x))) & 0xFFFFFFFF


def _percent(part, whole):
    return 0.0 if part == 0 or whole <= 0 else (float(part) / float(whole)) * 100.0


def _gc_text(st, length):
    den = length - int(st["n_bases"])
    return "-nan" if den == 0 else "%.5f" % (float(int(st["gc_bases"])) / float(den))


def _tail(st, length, k):
    nb = length - k + 1
    inv, nz = int(st["invalid"]), int(st["non_zero"])
    return "%d\t%d\t%d\t%.5f\t%d\t%.5f\t%.5f" % (length, (length - k + 1) & 0xFFFFFFFF, inv, _percent(inv, nb), nz, _percent(nz, nb),
                                                _percent(nz, nb - inv))


def sect_row(name, length, k, st):
    nb = length - k + 1
    mean = float(int(st["sum"])) / float(nb) if nb > 0 else 0.0
    med = _u32_of_double(st["median"]) if nb > 0 else 0
    return name + ("\t%d\t%.5f\t%s\t%s\n" % (med, mean, _gc_text(st, length), _tail(st, length, k))).encode()


def cold_row(name, length, k, st_reads, st_asm):
    nb = length - k + 1
    mean = float(int(st_reads["sum"])) / float(nb) if nb > 0 else 0.0
    med = _u32_of_double(st_reads["median"]) if nb > 0 else 0
    cn = _u32_of_double(st_asm["median"]) if nb > 0 else 0
    return name + ("\t%d\t%.5f\t%d\t%s\t%s\n" % (med, mean, cn, _gc_text(st_reads, length), _tail(st_reads, length, k))).encode()


def join_records(seqs):
    """The buffer the host mirror builds: records joined by newlines; (bytes, starts, lengths)."""
    starts, pos = [], 0
    for s in seqs:
        starts.append(pos)
        pos += len(s) + 1
    return b"".join(s + b"\n" for s in seqs), np.array(starts, np.uint64), np.array([len(s) for s in seqs], np.uint64)
