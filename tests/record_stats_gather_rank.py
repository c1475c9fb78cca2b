"""One rank of tests/test_gpu_record_stats_gather.py: the tables, ownership plans and ~3000-base sequence of tests/profile_gather_rank.py,
exchanged by owner (katgpu_exchange_merge), then katgpu_table_record_stats_gathered_host (kg_per_record.hip) over the records the
sequence's "\\n" bytes cut it into, every rank passing the same bases, records and ranges.  One communicator goes through every plan;
the load-time hooks (KATGPU_TEST_GATHER_BATCH, KATGPU_TEST_STATS_SHORT, KATGPU_TEST_STATS_BATCH) are the same for all.
argv: rank world id_file out_dir k mode
  mode  plans / plans_nc: canonical / non-canonical tables.  Per plan i rank 0 saves case_<i>.npz (stats, r0, r1) and prints the plan's
                  name; KATGPU_TIMING=1 puts its profile_gathered and record_stats_gathered lines before that
        mismatch: the last rank passes one record fewer -- KATGPU_ERR_INVALID_ARG on every rank, the communicator still carries an
                  all-reduce, and the call then goes through (after_mismatch.npz)
        nomem:    KATGPU_TEST_GATHER_NOMEM names a rank that reports it could not allocate: KATGPU_ERR_NOMEM on every rank, idem
        empty:    no records -- KATGPU_OK everywhere
        short:    k - 1 bases holding two records: their base classes are right, and nothing is gathered
The test imports records() and RANGES to know what every rank asked for."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kat_amd  # noqa: E402
from tests import profile_gather_rank as pr  # noqa: E402

U64 = np.uint64
RANGES = [(1, 2500), (2500, 0)]


def records(seq):
    """(starts, lengths) of the records of seq: what lies between its "\\n" bytes, the empty ones included."""
    parts = seq.split("\n")
    lens = np.array([len(p) for p in parts], U64)
    starts = np.concatenate([[0], np.cumsum(lens[:-1] + U64(1))]).astype(U64)
    return starts, lens


def short_case(k):
    """k - 1 bases, two records"""
    b = ("GC" + "ACGTN" * 13)[:k - 1]
    a = (k - 1) // 2
    return b, np.array([0, a], U64), np.array([a, k - 1 - a], U64)


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
    S, cases = pr.plans(k, world, canonical)

    def table(strings, cnt):
        t = eng.table(k, canonical, size_hint=size_hint)
        if len(strings):
            hi, lo = pr.keys(strings, k)
            if wide:
                t.merge_host_wide(hi, lo, cnt)
            else:
                t.merge_host(lo, cnt)
        return t

    def sum_still_works():
        assert int(comm.allreduce_u64([np.array([rank + 1], U64)])[0][0]) == world * (world + 1) // 2

    def save(name, got):
        stats, (r0, r1) = got
        np.savez(os.path.join(out_dir, name), stats=stats, r0=r0, r1=r1)

    if mode in ("plans", "plans_nc"):
        for ci, (name, plan, chosen) in enumerate(cases):
            t = table(*plan[rank])
            comm.exchange_merge(t)
            seq, _ = pr.sequence(k, S, chosen, canonical)
            st, ln = records(seq)
            got = comm.record_stats_gathered(t, seq, st, ln, RANGES, canonical)
            if rank == 0:
                save("case_%02d.npz" % ci, got)
                sys.stderr.flush()
                print("plan %02d %s slot_bytes %d" % (ci, name, t.slot_bytes()), flush=True)
            else:
                assert got is None
            t.free()
    else:
        name, plan, chosen = cases[0]
        t = table(*plan[rank])
        comm.exchange_merge(t)
        seq, _ = pr.sequence(k, S, chosen, canonical)
        st, ln = records(seq)
        b = np.frombuffer(seq.encode(), np.uint8)
        L = eng.L
        if mode == "mismatch":
            m = st.size - (1 if rank == world - 1 else 0)
            out = np.zeros(st.size, kat_amd.binding.RECORD_STATS)
            rc = L.katgpu_table_record_stats_gathered_host(comm.h, t.h, b.ctypes.data, b.size, st.ctypes.data, ln.ctypes.data, m, 1, None, 0,
                                                           out.ctypes.data, None, None)
            assert rc == 1, (rank, rc)                    # KATGPU_ERR_INVALID_ARG
            assert not out.view(U64).any()
            sum_still_works()
            got = comm.record_stats_gathered(t, seq, st, ln, RANGES, canonical)      # ... and the call itself goes through afterwards
            if rank == 0:
                save("after_mismatch.npz", got)
            print("mismatch ok rank %d" % rank)
        elif mode == "nomem":
            try:
                comm.record_stats_gathered(t, seq, st, ln, RANGES, canonical)
                raise SystemExit("rank %d: the call went through" % rank)
            except kat_amd.KatGpuError as e:
                assert e.code == 5, (rank, e.code, e.message)
                assert rank == int(os.environ["KATGPU_TEST_GATHER_NOMEM"]) or "rank %s " % os.environ["KATGPU_TEST_GATHER_NOMEM"] in e.message, e.message
            sum_still_works()
            print("nomem ok rank %d" % rank)
        elif mode == "empty":
            got = comm.record_stats_gathered(t, seq, [], [], RANGES, canonical)
            if rank == 0:
                assert got[0].shape == (0,) and [r.shape for r in got[1]] == [(0, 3), (0, 3)]
            else:
                assert got is None
            got = comm.record_stats_gathered(t, b"", [], [], None, canonical)           # ... nor bases, nor ranges
            assert (got[0].shape == (0,) and got[1] == []) if rank == 0 else got is None
            sum_still_works()
            print("empty ok rank %d" % rank)
        elif mode == "short":
            sb, sst, sln = short_case(k)
            got = comm.record_stats_gathered(t, sb, sst, sln, RANGES, canonical)
            if rank == 0:
                save("short.npz", got)
            else:
                assert got is None
            print("short ok rank %d" % rank)
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
