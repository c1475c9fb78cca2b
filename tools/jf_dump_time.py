#!/usr/bin/env python3
"""Time Table.dump_jf at a size where the writer matters: a table of about 2^LOG2 distinct k-mers (a synthetic genome counted on
the device; --k, 27 by default, above 32 for a two-word table), dumped to a memory-backed directory.  Prints one JSON line: the
median of --runs dumps after --warmup, the library's own katgpu_timing breakdown of the median run, every run in the order it was
made (seconds, breakdown, the process's peak resident set after it), the time a plain write of the same number of bytes to the same
place takes (the floor), and the peak resident set before and after the dumps.  Not a test and not read by bench.py.

To time another checkout of the library, put it first on PYTHONPATH: this script only appends its own tree to sys.path."""
import argparse
import json
import os
import re
import resource
import statistics
import sys
import tempfile
import time

os.environ.setdefault("KATGPU_TIMING", "1")
sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kat_amd  # noqa: E402


def timed_dump(table, path):
    """(seconds, the katgpu_timing jf_dump object or None): the library writes its line to the C stderr."""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as cap:
        saved = os.dup(2)
        os.dup2(cap.fileno(), 2)
        try:
            t0 = time.perf_counter()
            table.dump_jf(path)
            dt = time.perf_counter() - t0
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        cap.seek(0)
        text = cap.read().decode(errors="replace")
    m = re.search(r'katgpu_timing (\{"phase": "jf_dump".*\})', text)
    return dt, json.loads(m.group(1)) if m else None


def plain_write(path, nbytes, chunk=64 << 20):
    buf = memoryview(bytearray(os.urandom(1 << 20) * (chunk >> 20)))
    t0 = time.perf_counter()
    with open(path, "wb") as f:
        left = nbytes
        while left:
            n = min(left, chunk)
            f.write(buf[:n])
            left -= n
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2", type=int, default=27, help="the genome has 2^LOG2 bases")
    ap.add_argument("--k", type=int, default=27, help="k-mer length; 33 to 63 gives a two-word table of the same genome")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dir", default="/dev/shm")
    a = ap.parse_args()
    eng = kat_amd.Engine(0)
    n_bases = 1 << a.log2
    g = eng.synth_genome(n_bases, seed=5)
    t = eng.table(a.k, True, size_hint=2 * n_bases).count_bases(g)
    g.free()
    distinct = t.stats(want_total=False)["distinct"]
    path = os.path.join(a.dir, "jf_dump_time.%d.jf%d" % (os.getpid(), a.k))
    rss0 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    try:
        for _ in range(a.warmup):
            timed_dump(t, path)
        each = [timed_dump(t, path) + (resource.getrusage(resource.RUSAGE_SELF).ru_maxrss,) for _ in range(a.runs)]
        runs = sorted(each, key=lambda x: x[0])
        rss1 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
        nbytes = os.path.getsize(path)
        floor = statistics.median(plain_write(path, nbytes) for _ in range(max(a.runs, 1)))
    finally:
        if os.path.exists(path):
            os.unlink(path)
    med = runs[(len(runs) - 1) // 2]
    print(json.dumps({"tool": "jf_dump_time", "k": a.k, "distinct": distinct, "slot_bytes": t.slot_bytes(), "file_bytes": nbytes, "runs": a.runs, "warmup": a.warmup,
                      "dump_s_median": round(med[0], 3), "dump_s_all": [round(x[0], 3) for x in runs], "breakdown": med[1],
                      "each_run": [{"dump_s": round(x[0], 3), "breakdown": x[1], "ru_maxrss_kb": x[2]} for x in each],
                      "plain_write_s_median": round(floor, 3), "ru_maxrss_before_kb": rss0, "ru_maxrss_after_kb": rss1}))
    t.free()
    eng.close()


if __name__ == "__main__":
    main()
