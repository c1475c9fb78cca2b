"""Calls of the reference's own code (oracle/_ref: jf_ref, kat_ref_parts, seqan_ref -- built by `make -C oracle ref` only where the
reference's sources lie) -- and, where those binaries are not built, what they printed for the same call, replayed from
tests/golden/ref_calls/*.json.gz.  A call is keyed by the binary, its arguments, its stdin and the CONTENTS of the files it names
(repository and file directories written as placeholders; a .gz file by what it holds; the host, time and working directory a .jf
header records left out), so a
replayed answer is the one the real code gave for identical input.  Answers of up to KEEP bytes are stored whole; of a longer one only
its sha256 is, and the caller rebuilds the text (the oracle's k-mer dump, jfread_text below) -- returned only when its digest is the
reference's.  A call that was never recorded fails the test: the inputs changed, and the answers must be taken again with the binaries
present:

    KATGPU_RECORD_REF_CALLS=/path/calls.jsonl python -m pytest tests ...    # appends every real call
    python tests/refcalls.py /path/calls.jsonl ...                           # merges them into tests/golden/ref_calls/
"""
import glob
import gzip
import hashlib
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
JF_REF = os.path.join(REF_DIR, "jf_ref")
KAT_REF = os.path.join(REF_DIR, "kat_ref_parts")
SEQAN_REF = os.path.join(REF_DIR, "seqan_ref")
STORE = os.path.join(ROOT, "tests", "golden", "ref_calls")
SHARDS = 16
KEEP = 96 << 10
_VOLATILE_JF = ("time", "hostname", "pwd", "exe_path", "cmdline")
_cache = None


def built(binary):
    return os.access(binary, os.X_OK) and not os.environ.get("KATGPU_TEST_REPLAY_REF")


def _subs(args):
    """(real prefix, placeholder) pairs, longest first: the directories of the files named, the repository, the working directory."""
    dirs = {os.path.dirname(os.path.abspath(a)) for a in args if os.path.isfile(a)}
    pairs = [(d, "<DIR%d>" % i) for i, d in enumerate(sorted(dirs))] + [(ROOT, "<ROOT>"), (os.getcwd(), "<CWD>")]
    return sorted(((p.encode(), q.encode()) for p, q in pairs if p not in ("", "/")), key=lambda x: -len(x[0]))


def _norm(b, subs):
    for p, q in subs:
        b = b.replace(p, q)
    return b


def _file_digest(path, subs):
    data = open(path, "rb").read()
    if data[:2] == b"\x1f\x8b":                             # gzip: what it holds (its header carries a time stamp)
        data = b"gz\0" + gzip.decompress(data)
    m = re.match(rb"(\d{9})\{", data)
    if m:                                                  # a Jellyfish file: the header's fields, less the volatile ones, then the body
        n = int(m.group(1))
        try:
            hdr = json.loads(data[9:9 + n].rstrip(b"\0 \n").decode())
            for f in _VOLATILE_JF:
                hdr.pop(f, None)
            data = json.dumps(hdr, sort_keys=True).encode() + b"\0" + data[9 + n:]
        except ValueError:
            pass
    return hashlib.sha256(_norm(data, subs)).hexdigest()


def _key(binary, args, stdin, subs):
    parts = [os.path.basename(binary)]
    for a in args:
        parts.append("file:" + _file_digest(a, subs) if os.path.isfile(a) else _norm(a.encode(), subs).decode("latin-1"))
    parts.append(hashlib.sha256(_norm(stdin or b"", subs)).hexdigest())
    return hashlib.sha256("\0".join(parts).encode()).hexdigest()


def _load():
    global _cache
    if _cache is None:
        _cache = {}
        for f in glob.glob(os.path.join(STORE, "*.json.gz")):
            with gzip.open(f, "rt") as fh:
                _cache.update(json.load(fh))
    return _cache


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def _jf_offset(args):
    """jfread prints the header's length ("offset"), which follows the host / time / directory fields the key leaves out: stored as a
    placeholder, put back from the file itself."""
    if args[:1] == ["jfread"] and len(args) > 1 and os.path.isfile(args[1]):
        with open(args[1], "rb") as fh:
            head = fh.read(9)
        if head.isdigit():
            return b"\noffset %d\n" % (9 + int(head))
    return None


def _out_norm(out, args, subs):
    out = _norm(out, subs)
    off = _jf_offset(args)
    return out.replace(off, b"\noffset <OFFSET>\n", 1) if off else out


def run(binary, args, stdin=None, timeout=300, rebuild=None):
    """(exit status, stdout) of the reference binary on these arguments -- run, or replayed where it is not built.  rebuild(): the
    caller's own statement of the answer, used when only the answer's digest was stored; a text whose digest differs comes back as a
    marker that equals no answer."""
    args = [str(a) for a in args]
    subs = _subs(args)
    if built(binary):
        r = subprocess.run([binary] + args, input=stdin, capture_output=True, timeout=timeout)
        rec = os.environ.get("KATGPU_RECORD_REF_CALLS")
        if rec:
            with open(rec, "a") as fh:
                out = _out_norm(r.stdout, args, subs)
                e = {"key": _key(binary, args, stdin, subs), "rc": r.returncode, "sha256": _sha(out)}
                if len(out) <= KEEP:
                    e["out"] = out.decode("latin-1")
                fh.write(json.dumps(e) + "\n")
        return r.returncode, r.stdout
    e = _load().get(_key(binary, args, stdin, subs))
    if e is None:
        import pytest
        pytest.fail("%s %s: no recorded answer of the reference's code for these inputs, and oracle/_ref is not built (see tests/refcalls.py)"
                    % (os.path.basename(binary), " ".join(args)[:200]))
    if "out" not in e:
        if rebuild is None:
            import pytest
            pytest.fail("%s %s: only the digest of the reference's answer is stored, and the caller cannot rebuild it" % (os.path.basename(binary), " ".join(args)[:200]))
        out = rebuild()
        if _sha(_out_norm(out, args, subs)) != e["sha256"]:
            out = b"(not the reference's answer: its sha256 is %s)\n" % e["sha256"].encode()
        return e["rc"], out
    out = e["out"].encode("latin-1")
    for p, q in subs:                                        # the placeholders back to this checkout's paths
        out = out.replace(q, p)
    off = _jf_offset(args)
    return e["rc"], out.replace(b"\noffset <OFFSET>\n", off, 1) if off else out


def jfread_text(path):
    """What `jf_ref jfread <path>` prints, restated for a binary/sorted file: the header fields, then "<k-mer> <count> <position>" per record,
    the position being the header's hash matrix times the key (kat_amd/csrc/kg_jf.cpp: matrix_times) within the table size."""
    data = open(path, "rb").read()
    n = int(data[:9])
    hdr = json.loads(data[9:9 + n].rstrip(b"\0 \n").decode())
    key_len, counter_len, size = hdr["key_len"], hdr["counter_len"], hdr["size"]
    cols = hdr["matrix1"]["columns"]
    k, kb = key_len // 2, (key_len + 7) // 8
    lines = ["format %s" % hdr["format"], "key_len %d" % key_len, "val_len %d" % hdr["val_len"], "counter_len %d" % counter_len, "size %d" % size,
             "max_reprobe %d" % hdr["max_reprobe"], "canonical %d" % int(bool(hdr.get("canonical"))), "offset %d" % (9 + n)]
    rec = kb + counter_len
    for off in range(9 + n, len(data) - rec + 1, rec):
        key = int.from_bytes(data[off:off + kb], "little")
        count = int.from_bytes(data[off + kb:off + rec], "little")
        pos, x, i = 0, key, 0
        while x and i < len(cols):
            if x & 1:
                pos ^= cols[len(cols) - 1 - i]
            x >>= 1
            i += 1
        mer = "".join("ACGT"[(key >> (2 * (k - 1 - j))) & 3] for j in range(k))
        lines.append("%s %d %d" % (mer, count, pos & (size - 1)))
    return ("\n".join(lines) + "\n").encode()


def merge(paths):
    """Recorded calls (.jsonl) -> tests/golden/ref_calls/NN.json.gz, sharded by key."""
    entries = dict(_load())
    for p in paths:
        for line in open(p):
            e = json.loads(line)
            entries[e["key"]] = {q: e[q] for q in ("rc", "sha256", "out") if q in e}
    os.makedirs(STORE, exist_ok=True)
    for s in range(SHARDS):
        part = {k: v for k, v in sorted(entries.items()) if int(k[:2], 16) % SHARDS == s}
        with open(os.path.join(STORE, "%02d.json.gz" % s), "wb") as fh:
            with gzip.GzipFile(fileobj=fh, mode="wb", mtime=0) as gz:
                gz.write(json.dumps(part, sort_keys=True).encode())
    print("%d calls in %s" % (len(entries), STORE))


if __name__ == "__main__":
    merge(sys.argv[1:])
