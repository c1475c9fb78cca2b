"""One rank of tests/test_gpu_seq_hits_gather.py: tables filled from a plan and exchanged by owner, as tests/profile_gather_rank.py does
(its plans(), sequence(), owner() and keys() are used here), then asked for per-record hits with katgpu_table_seq_hits_gathered_host
(kg_query.hip), every rank passing the same bases and records.  The records of a sequence are its pieces between "\\n", empty ones
included.  KATGPU_TEST_HITS_BATCH / KATGPU_TEST_HITS_RECS (read when the library loads) are the same for all ranks.
argv: rank world id_file out_dir k mode
  mode  plans / plans_nc: canonical / non-canonical tables.  Per plan i rank 0 saves case_<i>.npy (its hits) and prints the plan's name;
                  KATGPU_TIMING=1 puts its seq_hits_gathered line before that
        empties:  two records with 2100 empty ones between them: one chunk sees more records than it has LDS bins (empties.npy)
        mismatch: the last rank passes one record fewer -- KATGPU_ERR_INVALID_ARG on every rank, the communicator still carries an
                  all-reduce, and the call itself works afterwards (after_mismatch.npy)
        nomem:    KATGPU_TEST_HITS_GATHER_NOMEM names a rank that reports it could not allocate: KATGPU_ERR_NOMEM on every rank, idem
        zero:     n_rec == 0 -- every rank returns OK, nothing is written, no timing line"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kat_amd  # noqa: E402
from tests.profile_gather_rank import keys, plans, sequence  # noqa: E402

U64 = np.uint64
N_EMPTY = 2100                                          # more than the 2048 LDS bins of a chunk


def records(seq):
    """(starts, lengths) of the pieces of seq between "\\n" -- empty ones included."""
    starts, lens, at = [], [], 0
    for piece in seq.split("\n"):
        starts.append(at)
        lens.append(len(piece))
        at += len(piece) + 1
    return np.array(starts, U64), np.array(lens, U64)


def with_empties(seq):
    """(bases, starts, lengths): the two halves of seq (its "\\n" turned into N) as records 0 and N_EMPTY + 1, empty records between."""
    flat = seq.replace("\n", "N")
    half = len(flat) // 2
    starts = np.array([0] + [half] * N_EMPTY + [half], U64)
    lens = np.array([half] + [0] * N_EMPTY + [len(flat) - half], U64)
    return flat, starts, lens


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
            st, ln = records(seq)
            got = comm.seq_hits_gathered(t, seq, st, ln, canonical)       # (ranks other than 0 pass no room for the hits)
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
        st, ln = records(seq)
        b = np.frombuffer(seq.encode(), np.uint8)
        L = eng.L
        if mode == "empties":
            flat, est, eln = with_empties(seq)
            got = comm.seq_hits_gathered(t, flat, est, eln, canonical)
            if rank == 0:
                np.save(os.path.join(out_dir, "empties.npy"), got)
            print("empties ok rank %d" % rank)
        elif mode == "mismatch":
            out = np.zeros(st.size, U64)
            rc = L.katgpu_table_seq_hits_gathered_host(comm.h, t.h, b.ctypes.data, b.size, st.ctypes.data, ln.ctypes.data,
                                                       st.size - (1 if rank == world - 1 else 0), 1, out.ctypes.data)
            assert rc == 1, (rank, rc)                    # KATGPU_ERR_INVALID_ARG
            msg = L.katgpu_last_error(eng.h).decode()
            assert "rank %d" % (world - 1) in msg, msg
            assert not out.any()
            sum_still_works()
            got = comm.seq_hits_gathered(t, seq, st, ln, canonical)     # ... and the call itself goes through afterwards
            if rank == 0:
                np.save(os.path.join(out_dir, "after_mismatch.npy"), got)
            print("mismatch ok rank %d" % rank)
        elif mode == "nomem":
            try:
                comm.seq_hits_gathered(t, seq, st, ln, canonical)
                raise SystemExit("rank %d: the hits went through" % rank)
            except kat_amd.KatGpuError as e:
                assert e.code == 5, (rank, e.code, e.message)
                assert rank == int(os.environ["KATGPU_TEST_HITS_GATHER_NOMEM"]) or "rank %s " % os.environ["KATGPU_TEST_HITS_GATHER_NOMEM"] in e.message, e.message
            sum_still_works()
            print("nomem ok rank %d" % rank)
        elif mode == "zero":
            guard = np.full(8, 0xDEADBEEF, U64)
            eng._chk(L.katgpu_table_seq_hits_gathered_host(comm.h, t.h, b.ctypes.data, b.size, st.ctypes.data, ln.ctypes.data, 0, 1,
                                                           guard.ctypes.data if rank == 0 else None))
            eng._chk(L.katgpu_table_seq_hits_gathered_host(comm.h, t.h, None, 0, None, None, 0, 1, None))
            assert (guard == U64(0xDEADBEEF)).all(), "something was written"
            sum_still_works()
            print("zero ok rank %d" % rank)
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
