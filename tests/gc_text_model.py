"""The text of `kat sect -g`'s -counts.gc, built in Python from per-position G+C counts (Sect::printGCCounts and gcCountToPercentage,
src/sect.cc:348-370, without the ">name" line): what katgpu_record_gc_text_* must return, byte for byte.  `gcs[p]` is the int16 the
oracle's ko.profile gives for the window that starts at byte p of the buffer the records lie in: -1 for a window with a byte outside
ACGTacgt, else its number of G g C c.  Record r is bytes [rec_start[r], rec_start[r] + rec_len[r]) and has nb = rec_len - k + 1 windows
when rec_len >= k, none otherwise."""
import numpy as np

from tests.cvg_text_model import joined, read_fasta  # noqa: F401  (the same FASTA reading and joining)

INVALID = b"-0.1"


def window_text(g, k):
    """one window's string: "%.1f" of the percentage, "-0.1" for an invalid window"""
    return INVALID if g < 0 else ("%.1f" % ((g / k) * 100.0)).encode()


def record_text(gcs, k):
    """one record's line from the G+C counts of its windows"""
    strings = [window_text(g, k) for g in range(k + 1)] + [INVALID]          # [-1] is the invalid one
    return b" ".join(strings[g] for g in np.asarray(gcs, np.int64).tolist()) + b"\n" if len(gcs) else b"0.0\n"


def text(rec_start, rec_len, k, gcs):
    """(bytes, offsets u64[n_rec + 1]): the records' lines one after another, and where each starts"""
    parts, off = [], [0]
    for s, n in zip(np.asarray(rec_start, np.uint64).tolist(), np.asarray(rec_len, np.uint64).tolist()):
        nb = n - k + 1 if n >= k else 0
        parts.append(record_text(gcs[s:s + nb], k))
        off.append(off[-1] + len(parts[-1]))
    return b"".join(parts), np.array(off, np.uint64)


def gc_file(names, rec_start, rec_len, k, gcs):
    """the whole -counts.gc: ">name" and the record's line, record after record"""
    body, off = text(rec_start, rec_len, k, gcs)
    off = off.tolist()
    return b"".join(b">" + name + b"\n" + body[off[i]:off[i + 1]] for i, name in enumerate(names))


def oracle_gcs(ko, k, bases):
    """the per-position array of a buffer from the oracle: any empty table of the right k will do"""
    table = ko.WideTable(k, True) if k > 32 else ko.Table(k, True)
    return ko.profile(table, bytes(bases), True)[1]
