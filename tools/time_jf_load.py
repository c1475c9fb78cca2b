#!/usr/bin/env python3
"""Time Engine.load_jf at a size where the loader matters.  A fixed recipe: a synthetic genome of --bases bases (default 2^27 + 2^20:
at least 2^27 distinct 27-mers) is counted on the device, the table is dumped to a memory-backed directory, and the file is loaded
--runs times (default 3) with KATGPU_TIMING=1.  Prints one JSON line: every load's wall time, the library's own katgpu_timing
"jf_load" object per load where it prints one, the time a plain read of the file takes (the floor), and the process's peak
resident set before the first load and after the last.  Not a test and not read by bench.py.

To time another checkout of the library, put it first on PYTHONPATH: this script only appends its own tree to sys.path."""
import argparse
import json
import os
import re
import resource
import sys
import tempfile
import time

os.environ.setdefault("KATGPU_TIMING", "1")
sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kat_amd  # noqa: E402


def timed_load(eng, path):
    """(seconds, distinct, the katgpu_timing jf_load object or None): the library writes its line to the C stderr."""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as cap:
        saved = os.dup(2)
        os.dup2(cap.fileno(), 2)
        try:
            t0 = time.perf_counter()
            t = eng.load_jf(path)
            dt = time.perf_counter() - t0
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        cap.seek(0)
        text = cap.read().decode(errors="replace")
    distinct = t.stats(want_total=False)["distinct"]
    t.free()
    eng.release_scratch()
    m = re.search(r'katgpu_timing (\{"phase": "jf_load".*\})', text)
    return dt, distinct, json.loads(m.group(1)) if m else None


def plain_read(path, chunk=64 << 20):
    buf = bytearray(chunk)
    t0 = time.perf_counter()
    with open(path, "rb", buffering=0) as f:
        while f.readinto(buf):
            pass
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bases", type=int, default=(1 << 27) + (1 << 20))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dir", default="/dev/shm")
    a = ap.parse_args()
    eng = kat_amd.Engine(0)
    g = eng.synth_genome(a.bases, seed=5)
    t = eng.table(27, True, size_hint=2 * a.bases).count_bases_device(g.ptr, a.bases)
    g.free()
    distinct = t.stats(want_total=False)["distinct"]
    path = os.path.join(a.dir, "time_jf_load.%d.jf27" % os.getpid())
    try:
        t.dump_jf(path)
        t.free()
        eng.release_scratch()
        nbytes = os.path.getsize(path)
        rss0 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
        runs = [timed_load(eng, path) for _ in range(a.runs)]
        rss1 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
        floor = min(plain_read(path) for _ in range(max(a.runs, 1)))
    finally:
        if os.path.exists(path):
            os.unlink(path)
    assert all(r[1] == distinct for r in runs), (distinct, [r[1] for r in runs])
    print(json.dumps({"tool": "time_jf_load", "library": os.path.dirname(kat_amd.__file__), "distinct": distinct, "file_bytes": nbytes, "runs": a.runs,
                      "load_s": [round(r[0], 3) for r in runs], "breakdown": [r[2] for r in runs], "plain_read_s_min": round(floor, 3),
                      "ru_maxrss_before_kb": rss0, "ru_maxrss_after_kb": rss1}))
    eng.close()


if __name__ == "__main__":
    main()
