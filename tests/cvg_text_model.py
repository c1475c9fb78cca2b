"""The text of `kat sect`'s -counts.cvg, built in Python from per-position counts (Sect::printCounts, src/sect.cc:328-346, without the
">name" line): what katgpu_table_record_cvg_text_* must return, byte for byte.  `counts[p]` is the count of the window that starts at
byte p of the buffer the records lie in (the oracle's ko.profile of that buffer); record r is bytes [rec_start[r], rec_start[r] +
rec_len[r]) and has nb = rec_len - k + 1 windows when rec_len >= k, none otherwise."""
import numpy as np


def record_text(counts):
    """one record's line from the counts of its windows"""
    return (" ".join(map(str, np.asarray(counts, np.uint64).tolist())) + "\n" if len(counts) else "0\n").encode()


def text(rec_start, rec_len, k, counts):
    """(bytes, offsets u64[n_rec + 1]): the records' lines one after another, and where each starts"""
    parts, off = [], [0]
    for s, n in zip(np.asarray(rec_start, np.uint64).tolist(), np.asarray(rec_len, np.uint64).tolist()):
        nb = n - k + 1 if n >= k else 0
        parts.append(record_text(counts[s:s + nb]))
        off.append(off[-1] + len(parts[-1]))
    return b"".join(parts), np.array(off, np.uint64)


def cvg_file(names, rec_start, rec_len, k, counts):
    """the whole -counts.cvg: ">name" and the record's line, record after record"""
    body, off = text(rec_start, rec_len, k, counts)
    off = off.tolist()
    return b"".join(b">" + name + b"\n" + body[off[i]:off[i + 1]] for i, name in enumerate(names))


def read_fasta(path):
    """(names, sequences) of a FASTA file as bytes: a name is the whole line behind '>', a sequence its lines joined"""
    names, seqs = [], []
    with open(path, "rb") as f:
        for line in f.read().split(b"\n"):
            line = line.rstrip(b"\r")
            if line.startswith(b">"):
                names.append(line[1:]); seqs.append([])
            elif names:
                seqs[-1].append(line)
    return names, [b"".join(s) for s in seqs]


def joined(seqs):
    """(buffer u8, starts, lengths): the sequences with a newline behind each, as `katgpu sect` joins a batch"""
    lens = np.array([len(s) for s in seqs], np.uint64)
    starts = np.concatenate([[0], np.cumsum(lens + np.uint64(1))[:-1]]).astype(np.uint64) if len(seqs) else np.zeros(0, np.uint64)
    return np.frombuffer(b"".join(s + b"\n" for s in seqs), np.uint8), starts, lens
