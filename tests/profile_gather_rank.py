"""One rank of tests/test_gpu_profile_gather.py: tables filled from a plan (katgpu_table_merge_host[_wide]), exchanged by owner
(katgpu_exchange_merge), then probed window by window with katgpu_table_profile_gathered_host (kg_query.hip), every rank passing the
same sequence.  The plans decide which rank OWNS the k-mers (kdist.owner_of[_wide], as tests/jf_gather_rank.py chooses them):
everything on rank 0, everything on the last rank (rank 0's own run is empty in every batch), one rank empty, an even split, no k-mer
at all.  One communicator goes through every plan; KATGPU_TEST_GATHER_BATCH (read when the library loads) is the same for all.
argv: rank world id_file out_dir k mode
  mode  plans / plans_nc: canonical / non-canonical tables.  Per plan i rank 0 saves case_<i>.npy (its counts) and prints the plan's name;
                  KATGPU_TIMING=1 puts its profile_gathered line before that
        short:    n < k -- nothing is written, every rank returns OK
        mismatch: the ranks pass different n -- KATGPU_ERR_INVALID_ARG on every rank, and the communicator still carries an all-reduce
        nomem:    KATGPU_TEST_GATHER_NOMEM names a rank that reports it could not allocate: KATGPU_ERR_NOMEM on every rank, idem
The test imports plans() and sequence() to know what every rank inserted and asked for."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kat_amd  # noqa: E402
from kat_amd import dist as kdist  # noqa: E402
from tests import jf_gather_rank as jr  # noqa: E402
from tests import naive  # noqa: E402

U64 = np.uint64
SEED = 20261019
BIG = 2 ** 40                                           # a count the slot cannot hold: the side table's
PLAN_KMERS = 96                                         # k-mers of a plan: ~3000 bases at k = 27
N_RUN = 130                                             # a run of N that swallows a whole batch of 64 windows wherever it starts


def text(hi, lo, k):
    """The k-mer (hi, lo) as a string: two bits a base, the first base in the top pair (naive.pack is the inverse)."""
    v = (int(hi) << 64) | int(lo)
    s = "".join("ACGT"[(v >> (2 * (k - 1 - i))) & 3] for i in range(k))
    assert naive.pack(s) == v
    return s


def keys(strings, k):
    """(hi, lo) arrays of k-mer strings."""
    v = [naive.pack(s) for s in strings]
    return np.array([x >> 64 for x in v], U64), np.array([x & (2 ** 64 - 1) for x in v], U64)


def owner(strings, k, world):
    hi, lo = keys(strings, k)
    if k <= 32:
        return np.asarray(kdist.owner_of(lo, k, world))
    return np.asarray(kdist.owner_of_wide(hi, lo, k, world))


def plans(k, world, canonical):
    """[(name, [(k-mer strings, counts) per rank], the strings in plan order)]: what every rank INSERTS, dealt round robin, so every
    plan also moves records in the exchange; who owns a k-mer is the hash's business.  A canonical table is given canonical k-mers; a
    non-canonical one every other k-mer as the reverse complement of its canonical form -- the owner is that of the canonical form
    either way."""
    P = jr.pool(k)
    S = [text(h, l, k) for h, l in P[:4000]]
    if not canonical:
        S = [naive.revcomp(s) if i & 1 else s for i, s in enumerate(S)]
    own = owner(S, k, world)
    rng = np.random.default_rng(SEED + 7 * k + world)

    def deal(idx):
        idx = [int(i) for i in idx]
        cnt = rng.integers(1, 5000, size=len(idx), dtype=U64)
        if len(idx):
            cnt[len(idx) // 2] = BIG
        chosen = [S[i] for i in idx]
        return [(chosen[s::world], cnt[s::world]) for s in range(world)], chosen

    out = [("even",) + deal(range(PLAN_KMERS)),
           ("all_on_rank0",) + deal(np.flatnonzero(own == 0)[:PLAN_KMERS]),
           ("all_on_last",) + deal(np.flatnonzero(own == world - 1)[:PLAN_KMERS])]
    if world > 2:
        out.append(("rank1_empty",) + deal(np.flatnonzero(own != 1)[:PLAN_KMERS]))
    out.append(("nothing",) + deal([]))
    return S, out


def sequence(k, S, chosen, canonical):
    """About 3000 bases made of the plan's k-mers -- the pool's where the plan has none: N runs (one of N_RUN), lowercase bases, "\\n"
    record joins, a record shorter than k, one of exactly k, k-mers the plan does not hold, and a k-mer as its reverse complement (the second value: that string; what it must give is the test's to say)."""
    rng = np.random.default_rng(SEED + k + len(chosen))
    have = chosen if chosen else S[:PLAN_KMERS]
    absent = [s for s in S[-40:] if s not in set(chosen)]
    strand = next(s for s in have if naive.revcomp(s) != s and naive.revcomp(s) not in set(chosen))
    parts, total = [], 0
    i = 0
    while total < 3000:
        s = have[i % len(have)]
        what = i % 12
        if what == 3:
            s = s.lower()
        elif what == 5:
            s = s[:k // 2] + s[k // 2:].lower() + "N" * int(rng.integers(1, 4))
        elif what == 7 and absent:
            s = absent[i % len(absent)]
        elif what == 9:
            s = "\n" + s + "\n"                           # a record of exactly k: one window
        elif what == 11:
            s = s + "\n" + s[:k - 1] + "\n"               # ... and one shorter than k
        parts.append(s)
        total += len(s)
        i += 1
        if i == 20:
            parts.append("N" * N_RUN)
        if i == 30:
            parts.append("\n" + naive.revcomp(strand) + "\n")
    return "".join(parts), naive.revcomp(strand)


def main():
    rank, world, id_file, out_dir, k, mode = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], int(sys.argv[5]), sys.argv[6]
    wide = k > 32
    canonical = mode != "plans_nc"
    size_hint = int(os.environ.get("PROFILE_GATHER_SIZE_HINT", str(1 << 16)))
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
    S, cases = plans(k, world, canonical)

    def table(strings, cnt):
        t = eng.table(k, canonical, size_hint=size_hint)
        if len(strings):
            hi, lo = keys(strings, k)
            if wide:
                t.merge_host_wide(hi, lo, cnt)
            else:
                t.merge_host(lo, cnt)
        return t

    def sum_still_works():
        assert int(comm.allreduce_u64([np.array([rank + 1], U64)])[0][0]) == world * (world + 1) // 2

    if mode in ("plans", "plans_nc"):
        for ci, (name, plan, chosen) in enumerate(cases):
            t = table(*plan[rank])
            comm.exchange_merge(t)
            seq, _ = sequence(k, S, chosen, canonical)
            got = comm.profile_gathered(t, seq, canonical)
            if rank == 0:
                np.save(os.path.join(out_dir, "case_%02d.npy" % ci), got)
                sys.stderr.flush()
                print("plan %02d %s slot_bytes %d" % (ci, name, t.slot_bytes()), flush=True)
            else:
                assert got is None
            t.free()
    else:
        name, plan, chosen = cases[0]
        t = table(*plan[rank])
        comm.exchange_merge(t)
        seq, _ = sequence(k, S, chosen, canonical)
        b = np.frombuffer(seq.encode(), np.uint8)
        L = eng.L
        if mode == "short":
            guard = np.full(8, 0xDEADBEEF, U64)
            for n in (0, 1, k - 1):
                eng._chk(L.katgpu_table_profile_gathered_host(comm.h, t.h, b.ctypes.data, n, 1, guard.ctypes.data if rank == 0 else None))
            assert (guard == U64(0xDEADBEEF)).all(), "something was written"
            print("short ok rank %d" % rank)
        elif mode == "mismatch":
            out = np.zeros(b.size, U64)
            rc = L.katgpu_table_profile_gathered_host(comm.h, t.h, b.ctypes.data, b.size - (1 if rank == world - 1 else 0), 1, out.ctypes.data)
            assert rc == 1, (rank, rc)                    # KATGPU_ERR_INVALID_ARG
            assert not out.any()
            sum_still_works()
            got = comm.profile_gathered(t, seq, canonical)        # ... and the call itself goes through afterwards
            if rank == 0:
                np.save(os.path.join(out_dir, "after_mismatch.npy"), got)
            print("mismatch ok rank %d" % rank)
        elif mode == "nomem":
            try:
                comm.profile_gathered(t, seq, canonical)
                raise SystemExit("rank %d: the profile went through" % rank)
            except kat_amd.KatGpuError as e:
                assert e.code == 5, (rank, e.code, e.message)
                assert rank == int(os.environ["KATGPU_TEST_GATHER_NOMEM"]) or "rank %s " % os.environ["KATGPU_TEST_GATHER_NOMEM"] in e.message, e.message
            sum_still_works()
            print("nomem ok rank %d" % rank)
        else:
            raise SystemExit("unknown mode " + mode)
        t.free()
    if rank == 0:
        print("transport:", comm.transport)
    comm.barrier()
    comm.free()
    eng.close()


if __name__ == "__main__":
    main()
