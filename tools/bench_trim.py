#!/usr/bin/env python3
"""What a 5' trim costs from files to a histogram: `katgpu hist -m 27 --5ptrim 0 | 5` on a plain FASTQ pair and on a FASTA assembly, for
one or more builds of the CLI (say the parent commit's and this tree's), five fresh processes per arm, the arms taking turns and the
builds swapping places from one repetition to the next.

  python tools/bench_trim.py --dir /dev/shm/trim --build parent=/path/to/parent/kat_amd/bin/katgpu --build branch=kat_amd/bin/katgpu

Writes into --dir (tmpfs, so that the readers' source is memory) from the seeded device generator: a pair of 2 x 16 M reads x 150 bp
(2 x 5.1 GB) and a 200 Mbp assembly at 80 columns, and removes them afterwards.  Every run has KATGPU_TIMING=1 and a time limit of its
own; a build without the trim on its fast paths streams a trimmed file through one reader thread per file (kg_ingest.hpp: stream_group),
memchr and vector::insert over every byte, a few hundred MB/s at worst: 5 GB per thread stay well inside --limit's 600 s.
Prints ONE JSON line: every run (build, input, trim, wall seconds, exit code, the library's katgpu_timing lines about files, the sha1 of
the .hist file) and per arm the median and min - max, the checks of DESIGN.md section 6 beside them."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import kat_amd  # noqa: E402

K, L = 27, 150


def write_inputs(tmp, n_reads, genome, fasta_bases):
    eng = kat_amd.Engine(0)
    g = eng.synth_genome(genome, seed=4242)
    pair = [os.path.join(tmp, "lib_R%d.fastq" % m) for m in (1, 2)]
    files = [open(p, "wb") for p in pair]
    for lo in range(0, n_reads, 8_000_000):
        m = min(8_000_000, n_reads - lo)
        r = eng.synth_reads(g, genome, first_read=lo, n_reads=m, read_len=L, frag_len=350, err_ppm=2000, seed=7)
        h = r.download().reshape(m, L + 1)[:, :L]
        r.free()
        for mate in (0, 1):
            bench.write_fastq(files[mate], h[mate::2], lo // 2, mate, L)
    for f in files:
        f.close()
    g.free()
    a = eng.synth_genome(fasta_bases, seed=99)
    asm = a.download()
    a.free()
    eng.close()
    fa = os.path.join(tmp, "asm.fa")
    clen = 1_000_000
    with open(fa, "wb") as f:
        for c in range((fasta_bases + clen - 1) // clen):
            seq = asm[c * clen:(c + 1) * clen]
            f.write(b">contig%d\n" % c)
            pad = (-seq.size) % 80
            rows = np.concatenate([seq, np.full(pad, ord("\n"), np.uint8)]).reshape(-1, 80)
            f.write(np.concatenate([rows, np.full((rows.shape[0], 1), ord("\n"), np.uint8)], axis=1).tobytes().rstrip(b"\n") + b"\n")
    return {"pair": pair, "fasta": [fa]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", required=True, help="a directory on tmpfs with room for 11 GB")
    ap.add_argument("--build", action="append", required=True, help="NAME=path of a katgpu executable (repeat)")
    ap.add_argument("--reads", type=int, default=32_000_000, help="reads of the pair, both mates together")
    ap.add_argument("--fasta-bases", type=int, default=200_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--trims", default="0,5")
    ap.add_argument("--limit", type=float, default=600.0, help="seconds one run may take")
    a = ap.parse_args()
    builds = [b.split("=", 1) for b in a.build]
    trims = [int(t) for t in a.trims.split(",")]
    os.makedirs(a.dir, exist_ok=True)
    n = a.reads & ~1
    genome = 120_000_000
    inputs = write_inputs(a.dir, n, genome, a.fasta_bases)
    sizes = {i: sum(os.path.getsize(p) for p in ps) for i, ps in inputs.items()}
    hint = {"pair": int(bench.expected_distinct(n * (L - K + 1), genome, K, 2000) / 0.62) + (1 << 20), "fasta": int(a.fasta_bases / 0.62) + (1 << 20)}
    env = {k: v for k, v in os.environ.items() if not k.startswith("KATGPU_")}
    env["KATGPU_TIMING"] = "1"
    runs, failed = [], False
    try:
        for rep in range(a.runs):
            for inp, paths in inputs.items():
                for trim in trims:
                    # The arms take turns, and the builds swap places from one repetition to the next: a process that starts right after
                    # another has freed tens of GB of HBM pays for it in its first file ("Allocation order"), so
                    # whoever always ran second behind a large run would look slower than it is.  "after" names the run before.
                    for name, exe in builds[rep % len(builds):] + builds[:rep % len(builds)]:
                        if failed:
                            continue
                        out = os.path.join(a.dir, "out.hist")
                        cmd = [os.path.abspath(exe), "hist", "-m", str(K), "-H", str(hint[inp]), "--5ptrim", str(trim), "-o", out] + paths
                        t0 = time.perf_counter()
                        try:
                            pr = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.limit)
                            rc, err = pr.returncode, pr.stderr
                        except subprocess.TimeoutExpired as e:
                            rc, err = 124, e.stderr if isinstance(e.stderr, str) else (e.stderr or b"").decode(errors="replace")
                        wall = time.perf_counter() - t0
                        sha = None
                        if rc == 0:
                            with open(out, "rb") as f:
                                sha = hashlib.sha1(b"\n".join(ln for ln in f.read().split(b"\n") if not ln.startswith(b"#"))).hexdigest()
                            os.unlink(out)
                        runs.append({"build": name, "input": inp, "trim": trim, "rep": rep, "wall_s": round(wall, 3), "rc": rc, "hist_sha1": sha,
                                     "after": "%s/%s/trim%d" % (runs[-1]["build"], runs[-1]["input"], runs[-1]["trim"]) if runs else "the generator",
                                     "katgpu_timing": [ln[len("katgpu_timing "):] for ln in err.splitlines() if ln.startswith("katgpu_timing ")]})
                        print("%s %s trim %d run %d: %.2f s (rc %d)" % (name, inp, trim, rep, wall, rc), file=sys.stderr, flush=True)
                        if rc != 0:                               # a run that failed or ran out of time: nothing more is started
                            failed = True
                            print(err[-2000:], file=sys.stderr)
    finally:
        for paths in inputs.values():
            for p in paths:
                if os.path.exists(p):
                    os.unlink(p)
    arms = {}
    for r in runs:
        if r["rc"] == 0:
            arms.setdefault("%s/%s/trim%d" % (r["build"], r["input"], r["trim"]), []).append(r["wall_s"])
    summary = {k: {"median_s": round(statistics.median(v), 3), "min_s": min(v), "max_s": max(v), "runs": len(v)} for k, v in arms.items()}
    shas = {}
    for r in runs:
        shas.setdefault("%s/trim%d" % (r["input"], r["trim"]), set()).add(r["hist_sha1"])
    print(json.dumps({"tool": "bench_trim", "k": K, "reads": n, "read_len": L, "fasta_bases": a.fasta_bases, "bytes": sizes,
                      "builds": [b[0] for b in builds], "summary": summary, "hist_identical_across_builds_and_runs": {k: len(v) == 1 and None not in v for k, v in shas.items()},
                      "complete": not failed, "runs": runs}))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
