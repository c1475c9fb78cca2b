"""Diagnostic: the two `kat filter` kernels on the bench workload's table (config 4: 300 M reads of 150 bp from a 1 Gbp genome, k = 27).
    python tools/bench_filter.py [--reads N] [--genome G] [--hit-reads M]
filter kmer: katgpu_table_filter with `-s` (keep and drop tables), KAT's default box; ms and TB/s of table bytes read (the input's slots)
and written (the two new tables' slots, cleared then filled).  Read hits: katgpu_table_seq_hits_device over the first M reads as records,
against k_profile (8 bytes per position) on the same bytes -- the pair the new kernel replaces, before any host sum."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kat_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=300_000_000)
    ap.add_argument("--genome", type=int, default=1_000_000_000)
    ap.add_argument("--hit-reads", type=int, default=20_000_000)
    ap.add_argument("--k", type=int, default=27)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    eng = kat_amd.Engine(0)

    def say(m):
        eng.sync()
        print(m, file=sys.stderr, flush=True)

    g = eng.synth_genome(a.genome, seed=20260927)
    reads = eng.synth_reads(g, a.genome, first_read=0, n_reads=a.reads, read_len=150, frag_len=350, err_ppm=2000, seed=1)
    g.free()
    t = eng.table(a.k, True, size_hint=4928956472)      # the bench's config 4 hint (-H of its end-to-end leg)
    t.count_bases_device(reads.ptr, reads.nbytes)
    eng.release_scratch()
    st = t.stats()
    slot = t.slot_bytes()
    say("table: %s, %d B per slot" % (st, slot))

    runs = []
    for _ in range(a.reps):
        eng.sync()
        t0 = time.perf_counter()
        keep, drop, ctr = t.filter(separate=True)
        eng.sync()
        ms = (time.perf_counter() - t0) * 1e3
        keep.free(); drop.free()
        runs.append(ms)
    cap = st["capacity"]
    moved = cap * slot * 3                      # the input's slots read, two new tables' slots written
    best = min(runs)
    filt = {"ms": runs, "best_ms": best, "table_bytes_read_written": moved, "TB_per_s": moved / (best * 1e-3) / 1e12,
            "counters": ctr, "note": "wall time of katgpu_table_filter: two table allocations + clears, the pass, the counters' read-back"}
    say("filter: %s" % json.dumps(filt))

    # read hits on the first hit-reads reads (151 bytes each: the read and a newline), one record per read
    n = min(a.hit_reads, a.reads)
    nb = n * 151
    starts = np.arange(n, dtype=np.uint64) * np.uint64(151)
    lens = np.full(n, 150, np.uint64)
    rec = eng.alloc(3 * 8 * n)
    rec.upload(starts); rec.upload(lens, offset=8 * n)
    n_out = nb - a.k + 1
    prof = eng.alloc(n_out * 8)
    res = {}
    for name, fn in (("seq_hits", lambda: t.seq_hits_device(reads.ptr, nb, rec.ptr, rec.ptr + 8 * n, n, rec.ptr + 16 * n)),
                     ("profile", lambda: t.profile_device(reads.ptr, nb, prof))):
        fn()
        eng.sync()
        eng.profile_reset()
        for _ in range(a.reps):
            fn()
        eng.sync()
        p = eng.profile()["profile"]
        kms = p["ms"] / max(1, p["launches"])
        res[name] = {"kernel_ms": kms, "G_positions_per_s": n_out / (kms * 1e-3) / 1e9}
    hits = rec.download(np.uint64, n, offset=16 * n)
    t0 = time.perf_counter()
    pc = prof.download(np.uint64, min(n_out, 1 << 28))
    host = (pc.reshape(-1)[: (pc.size // 151) * 151].reshape(-1, 151)[:, :151 - a.k] > 0).sum(axis=1)
    res["profile"]["host_sum_ms_first_%d_reads" % host.size] = (time.perf_counter() - t0) * 1e3
    res["hits_match_profile_sum"] = bool(np.array_equal(hits[: host.size], host.astype(np.uint64)))
    print(json.dumps({"table": st, "slot_bytes": slot, "filter_kmer": filt, "read_hits": res, "hit_reads": n}))


if __name__ == "__main__":
    main()
