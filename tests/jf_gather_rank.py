"""One rank of tests/test_gpu_jf_gather.py: tables filled from a plan (katgpu_table_merge_host[_wide]), exchanged by owner
(katgpu_exchange_merge), then written as one .jf file by katgpu_jf_dump_gathered (kg_jf.cpp, jf_gather in kg_jf_device.hip).  The plans
decide which rank OWNS the k-mers (kdist.owner_of[_wide]): everything on rank 0, everything on the last rank (rank 0's own run is empty
in every range), one rank empty, an even split, no k-mer at all, a single one, a stretch of positions that holds no k-mer of any
rank, and -- at 64 records a range -- a last range that is empty on every rank.  One communicator goes through every plan;
KATGPU_JF_RANGE_RECORDS (read when the library loads) is the same for all of them.
argv: rank world id_file out_dir k mode
  mode  plans: per plan i, rank 0 writes case_<i>.jf (the gathered file) and case_<i>.single.jf (katgpu_jf_dump of one table that
               holds the union), and prints the plan's name; KATGPU_TIMING=1 puts rank 0's jf_dump_gathered lines beside them
        nomem: KATGPU_TEST_JF_GATHER_NOMEM names a rank that reports it could not allocate: every rank must get KATGPU_ERR_NOMEM, no
               file may appear, and the communicator must still carry an all-reduce
        noopen: rank 0's path lies in a directory that does not exist: every rank must get KATGPU_ERR_IO (rank 0 with the path, its
               peers naming rank 0), nothing may exist at the path, and the communicator must still carry an all-reduce
The test imports plans() to know what every rank inserted."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kat_amd  # noqa: E402
from kat_amd import dist as kdist  # noqa: E402

U64 = np.uint64
POOL, SEED = 40000, 20261018
SATURATING = (2 ** 32 - 1, 2 ** 32, 2 ** 40)           # counts that must appear as 0xFFFFFFFF (the first one is that already)
GAP_TOTAL = 1200                                        # records of the plan whose positions leave a stretch empty
TAIL_TOTAL, TAIL_PILE = 70, 66                          # the plan with an empty last range: 66 of its 70 records share one position, none lies above


def pool(k):
    """Distinct canonical k-mers, the same on every rank: an (n, 2) array of (hi, lo); all 512 of them at k = 5."""
    rng = np.random.default_rng(SEED + k)
    if k <= 32:
        x = np.arange(1 << (2 * k), dtype=U64) if k <= 8 else rng.integers(0, 1 << (2 * k), size=POOL, dtype=U64, endpoint=False)
        x = np.unique(np.minimum(x, kdist._revcomp(x, k)))
        x = x[rng.permutation(x.size)]
        return np.stack([np.zeros_like(x), x], axis=1)
    hi = rng.integers(0, 1 << (2 * k - 64), size=POOL, dtype=U64)
    lo = rng.integers(0, np.iinfo(U64).max, size=POOL, dtype=U64, endpoint=True)
    rhi, rlo = kdist._revcomp_wide(hi, lo, k)
    take_rc = (rhi < hi) | ((rhi == hi) & (rlo < lo))
    hi, lo = np.where(take_rc, rhi, hi), np.where(take_rc, rlo, lo)
    _, first = np.unique(hi.astype(object) * (1 << 64) + lo.astype(object), return_index=True)
    first = np.sort(first)
    return np.stack([hi[first], lo[first]], axis=1)


def owners(P, k, world):
    if k <= 32:
        return np.asarray(kdist.owner_of(P[:, 1], k, world))
    return np.asarray(kdist.owner_of_wide(P[:, 0], P[:, 1], k, world))


def header_matrix(path):
    """(r, the 2k columns) of a .jf file's "matrix1"."""
    import json
    raw = open(path, "rb").read()
    m = json.loads(raw[9:9 + int(raw[:9])].rstrip(b"\0"))["matrix1"]
    return int(m["r"]), [int(c) for c in m["columns"]]


def positions(P, cols, r):
    """(M * kmer) & (2^r - 1): bit i of the 2k-bit k-mer selects column 2k-1-i."""
    c = len(cols)
    pos = np.zeros(len(P), U64)
    for i in range(c):
        word, bit = (P[:, 1], i) if i < 64 else (P[:, 0], i - 64)
        pos ^= np.where((word >> U64(bit)) & U64(1), U64(cols[c - 1 - i]), U64(0)).astype(U64)
    return pos & U64((1 << r) - 1)


def write_host(path, k, P, counts):
    """The host writer (pinned to the reference's reader by tests/test_jf.py) on (hi, lo) keys."""
    if k > 32:
        kat_amd.jf_write_records_wide(path, k, True, P[:, 0], P[:, 1], counts)
    else:
        kat_amd.jf_write_records(path, k, True, P[:, 1], counts)


def plans(k, world, even_total, scratch_dir):
    """[(name, [(pool indices, counts) per rank])]: what every rank INSERTS; who owns a k-mer is the hash's business.  The inserting
    ranks are dealt round robin, so every plan also moves records in the exchange."""
    P = pool(k)
    own = owners(P, k, world)
    rng = np.random.default_rng(SEED + 7 * k + world)
    none = (np.zeros(0, np.int64), np.zeros(0, U64))

    def matrix_for(n):
        """(r, columns) of the header a file of n records of this k gets (the matrix is seeded by k and n): read from a file the host
        writer makes for any n k-mers."""
        probe = os.path.join(scratch_dir, "probe.%d.%d.%d.jf" % (k, n, os.getpid()))
        write_host(probe, k, P[:n], np.ones(n, U64))
        r, cols = header_matrix(probe)
        os.remove(probe)
        return r, cols

    def deal(idx, cnt=None):
        cnt = rng.integers(1, 5000, size=idx.size, dtype=U64) if cnt is None else cnt
        return [(idx[s::world], cnt[s::world]) for s in range(world)]

    out = []
    idx = np.arange(min(even_total, len(P)))
    cnt = rng.integers(1, 5000, size=idx.size, dtype=U64)
    cnt[:len(SATURATING)] = np.array(SATURATING, U64)
    out.append(("even", deal(idx, cnt)))
    out.append(("all_on_rank0", deal(np.flatnonzero(own == 0)[:900])))
    out.append(("all_on_last", deal(np.flatnonzero(own == world - 1)[:900])))
    if world > 2:
        out.append(("rank1_empty", deal(np.flatnonzero(own != 1)[:900])))
    out.append(("nothing", [none] * world))
    out.append(("single", deal(np.arange(3, 4))))
    # a quarter of the positions without a k-mer on any rank
    if len(P) >= 4 * GAP_TOTAL:
        r, cols = matrix_for(GAP_TOTAL)
        pos = positions(P, cols, r)
        keep = np.flatnonzero((pos < U64((1 << r) // 4)) | (pos >= U64((1 << r) // 2)))[:GAP_TOTAL]
        assert keep.size == GAP_TOTAL
        out.append(("gap", deal(keep)))
        # A range that is empty on EVERY rank.  The cut loop closes a range before the stretch that would take it past the target; a
        # stretch that holds more than the target by itself is closed by the (empty) stretch after it, and when nothing follows, the last
        # range -- from there to 2^r -- holds no record.  70 records make r = 8 and stretches of one position: 66 k-mers of one
        # position p in the middle, 4 below it, none above.  With 64 records a range the cuts are [0, p) with 4, [p, p + 1) with 66 and
        # [p + 1, 2^r) with none; with a larger target it is one range.
        r, cols = matrix_for(TAIL_TOTAL)
        pos = positions(P, cols, r)
        p = U64((1 << r) // 2)
        pile, below = np.flatnonzero(pos == p)[:TAIL_PILE], np.flatnonzero(pos < p)[:TAIL_TOTAL - TAIL_PILE]
        assert pile.size == TAIL_PILE and below.size == TAIL_TOTAL - TAIL_PILE, (pile.size, below.size)
        out.append(("empty_tail", deal(np.concatenate([below, pile]))))
    return P, out


def main():
    rank, world, id_file, out_dir, k, mode = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], int(sys.argv[5]), sys.argv[6]
    wide = k > 32
    eng = kat_amd.Engine(0)
    if rank == 0:
        cid = kat_amd.Comm.unique_id()
        with open(id_file + ".tmp", "wb") as f:
            f.write(cid)
        os.rename(id_file + ".tmp", id_file)
    else:
        t0 = time.time()
        while not os.path.exists(id_file):
            assert time.time() - t0 < 120, "no id from rank 0"
            time.sleep(0.01)
        cid = open(id_file, "rb").read()
    comm = kat_amd.Comm(eng, rank, world, cid)
    P, cases = plans(k, world, int(os.environ["JF_GATHER_EVEN_TOTAL"]), out_dir)

    def table(idx, cnt):
        t = eng.table(k, True, size_hint=1 << 16)
        if idx.size:
            if wide:
                t.merge_host_wide(P[idx, 0], P[idx, 1], cnt)
            else:
                t.merge_host(P[idx, 1], cnt)
        return t

    if mode == "nomem":
        name, plan = cases[0]
        t = table(*plan[rank])
        comm.exchange_merge(t)
        path = os.path.join(out_dir, "nomem.jf")
        try:
            comm.jf_dump_gathered(t, path)
            raise SystemExit("rank %d: the dump went through" % rank)
        except kat_amd.KatGpuError as e:
            assert e.code == 5, (rank, e.code, e.message)
            assert "rank %s " % os.environ["KATGPU_TEST_JF_GATHER_NOMEM"] in e.message, e.message
        comm.barrier()
        assert not os.path.exists(path), "a file was created"
        assert int(comm.allreduce_u64([np.array([rank + 1], U64)])[0][0]) == world * (world + 1) // 2
        print("nomem ok rank %d" % rank)
        t.free()
    elif mode == "noopen":
        name, plan = cases[0]
        t = table(*plan[rank])
        comm.exchange_merge(t)
        path = os.path.join(out_dir, "no_such_dir", "noopen.jf")
        try:
            comm.jf_dump_gathered(t, path)
            raise SystemExit("rank %d: the dump went through" % rank)
        except kat_amd.KatGpuError as e:
            assert e.code == 2, (rank, e.code, e.message)
            assert ("cannot open " + path if rank == 0 else "rank 0 cannot open the output file") in e.message, e.message
        comm.barrier()
        assert not os.path.lexists(path) and not os.path.lexists(os.path.dirname(path)), "something was created"
        assert int(comm.allreduce_u64([np.array([rank + 1], U64)])[0][0]) == world * (world + 1) // 2
        print("noopen ok rank %d" % rank)
        t.free()
    else:
        for ci, (name, plan) in enumerate(cases):
            t = table(*plan[rank])
            comm.exchange_merge(t)
            comm.jf_dump_gathered(t, os.path.join(out_dir, "case_%02d.jf" % ci))
            t.free()
            if rank == 0:
                sys.stderr.flush()
                print("plan %02d %s" % (ci, name), flush=True)
                u = table(np.concatenate([p[0] for p in plan]), np.concatenate([p[1] for p in plan]))
                u.dump_jf(os.path.join(out_dir, "case_%02d.single.jf" % ci))
                u.free()
        if rank == 0:
            print("plans:", len(cases), "| transport:", comm.transport)
    comm.barrier()
    comm.free()
    eng.close()


if __name__ == "__main__":
    main()
