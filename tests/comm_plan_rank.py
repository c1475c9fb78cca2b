"""One rank of tests/test_gpu_comm_small.py: tables filled from a plan (katgpu_table_merge_host), not by counting reads, so that every
send list, receive set and chunk of the exchange (kg_comm.hip: katgpu_exchange_merge, _begin / _finish) holds an exact, small number of
records -- none, one, 31, 32, 33, ... -- or only records that travel out of band.  One communicator goes through every size case.
Every rank builds the same plans: one pool of canonical k-mers, every rank's table geometry (shared by an all-reduce), owners by
kdist.owner_of, regions by katgpu_place_keys, chunks as Exchange::cut cuts them (region bounds i * R / C of the sender's grid).
argv: rank world id_file out_dir form shape
  form   packed (k = 27, regions of 128 slots: 9-byte records), wire12 (the same tables, 12-byte records), mixed (rank 1 has another
         grid: the direct path), xs (k = 29, packed, remainders of more than 40 bits: the count word carries their top bits), wide (k = 45)
  shape  pipelined (katgpu_exchange_merge) or split (katgpu_exchange_begin / _finish)
Writes case_<i>.rank<r>.npz per case: what the rank inserted into both tables, what table 1 holds after the exchange, the all-reduced
hist / gcp / comp, and whether the records travelled packed."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kat_amd  # noqa: E402
from kat_amd import binding as kb  # noqa: E402
from kat_amd import dist as kdist  # noqa: E402

K = {"packed": 27, "wire12": 27, "mixed": 27, "xs": 29, "wide": 45}
TOTAL_SEND = (1, 31, 32, 33, 64, 85, 86, 300)
CHUNK_IN = (0, 1, 32, 33)
POOL, SEED = 60000, 20261016


def hint_of(form, rank):
    if form == "mixed" and rank == 1:
        return 1 << 24
    return {"xs": 1 << 21, "wide": 1 << 20}.get(form, 1 << 22)


def pool(k):
    """Distinct canonical k-mers, the same on every rank: uint64 keys, or (hi, lo) for k > 32."""
    rng = np.random.default_rng(SEED)
    if k <= 32:
        x = rng.integers(0, 1 << (2 * k), size=POOL, dtype=np.uint64)
        x = np.unique(np.minimum(x, kdist._revcomp(x, k)))
        return x[rng.permutation(x.size)]
    hi = rng.integers(0, 1 << (2 * k - 64), size=POOL, dtype=np.uint64)
    lo = rng.integers(0, np.iinfo(np.uint64).max, size=POOL, dtype=np.uint64, endpoint=True)
    rhi, rlo = kdist._revcomp_wide(hi, lo, k)
    take_rc = (rhi < hi) | ((rhi == hi) & (rlo < lo))
    hi, lo = np.where(take_rc, rhi, hi), np.where(take_rc, rlo, lo)
    _, first = np.unique(hi.astype(object) * (1 << 64) + lo.astype(object), return_index=True)
    first = np.sort(first)
    return np.stack([hi[first], lo[first]], axis=1)


def owners(keys, k, world):
    if k <= 32:
        return kdist.owner_of(keys, k, world)
    return kdist.owner_of_wide(keys[:, 0], keys[:, 1], k, world)


def main():
    rank, world, id_file, out_dir, form, shape = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5], sys.argv[6]
    k = K[form]
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

    # every rank's grid: a table made first (the geometry depends on KATGPU_TEST_REGION_SLOTS, read when the library loads)
    probe = eng.table(k, True, size_hint=hint_of(form, rank))
    geo = np.zeros((world, 3), np.uint64)
    xs = 0
    if not wide:
        g = probe.geometry()
        geo[rank] = (g.n_regions, g.p1, g.p2)
    probe.free()
    geo = comm.allreduce_u64([geo])[0].astype(np.int64)
    P = pool(k)
    own = owners(P, k, world)
    C = 1
    chunk = np.zeros((world, len(P)), np.int64)                       # chunk of each pool key in sender s's grid
    if not wide:
        C = max(1, min(int(os.environ.get("KATGPU_TEST_EXCHANGE_CHUNKS", "4")), int(geo[:, 0].min())))
        for s in range(world):
            R, p1, p2 = (int(v) for v in geo[s])
            d1, d2, _, _, rb = kb.place_keys(k, p1, p2.bit_length() - 1, P)
            region = d1.astype(np.int64) * p2 + d2
            bounds = np.array([i * R // C for i in range(C + 1)], np.int64)
            chunk[s] = np.searchsorted(bounds, region, side="right") - 1
            if s == rank:
                xs = max(rb, 40) - 40

    used = np.zeros(len(P), bool)

    def take(n, mask=None):
        """n unused pool keys (indices), where `mask` holds."""
        ok = ~used if mask is None else (~used & mask)
        idx = np.flatnonzero(ok)[:n]
        assert idx.size == n, ("pool too small", n, idx.size)
        used[idx] = True
        return idx

    rng = np.random.default_rng(SEED + 1)

    def counts(n):
        return rng.integers(1, 5000, size=n, dtype=np.uint64)

    # the cases: per rank, (pool indices, counts)
    cases = []
    cases.append([(np.zeros(0, np.int64), np.zeros(0, np.uint64)) for _ in range(world)])                   # every rank empty
    c = [(np.zeros(0, np.int64), np.zeros(0, np.uint64)) for _ in range(world)]
    if world > 1:                                                                                          # one rank empty, one with 1 record
        i = take(1)
        c[world - 1] = (i, counts(1))
    else:
        i = take(1)
        c[0] = (i, counts(1))
    cases.append(c)
    for n in TOTAL_SEND:                                                                                   # a send list of n records per rank
        cases.append([(lambda i: (i, counts(len(i))))(take(n)) for _ in range(world)])
    if not wide:                                                                                           # chunk_in(i) in {0, 1, 32, 33}, some chunks empty
        c = []
        for s in range(world):
            r = (s + world - 1) % world                                                                    # rank s sends to r only (itself with one rank)
            idx = np.concatenate([take(CHUNK_IN[i % len(CHUNK_IN)], (own == r) & (chunk[s] == i)) for i in range(C)])
            c.append((idx, counts(idx.size)))
        cases.append(c)
    cases.append([(lambda i: (i, counts(len(i))))(take(40, own == 0)) for _ in range(world)])              # everything owned by rank 0
    same = take(50)
    cases.append([(same, counts(50)) for _ in range(world)])                                              # the same keys on every rank: the owner sums them
    c = []                                                                                                 # rank 0's only records travel out of band
    for s in range(world):
        if s == 0:
            i = take(2)
            c.append((i, np.array([(1 << 32) + 3, (1 << 33) + 7], np.uint64)))
        else:
            i = take(10)
            c.append((i, counts(10)))
    cases.append(c)
    if xs:                                                                                                 # rank 0's only records: counts past the packed record's 32 - xs bits, inside 32
        c = []
        for s in range(world):
            i = take(2)
            c.append((i, np.array([(1 << (32 - xs)) + 1, (1 << 32) - 1], np.uint64) if s == 0 else counts(2)))
        cases.append(c)

    def fill(t, idx, cnt):
        if not idx.size:
            return
        if wide:
            t.merge_host_wide(P[idx, 0], P[idx, 1], cnt)
        else:
            t.merge_host(P[idx], cnt)

    for ci, plan in enumerate(cases):
        idx, cnt = plan[rank]
        idx2 = idx[::2]
        cnt2 = (cnt[::2] % np.uint64(7)) + np.uint64(1)
        t1 = eng.table(k, True, size_hint=hint_of(form, rank))
        t2 = eng.table(k, True, size_hint=hint_of(form, rank), like=None if wide else t1)
        fill(t1, idx, cnt)
        fill(t2, idx2, cnt2)
        if shape == "split":
            comm.exchange_begin(t1)
            comm.exchange_finish(t1)
        else:
            comm.exchange_merge(t1)
        packed = comm.stats()["records_packed"]
        got = t1.dump_sorted()
        comm.exchange_merge(t2)
        mx, cc, sp = kat_amd.comp(t1, t2, 1.0, 1.0, 201, 101)
        h, gm = t1.hist(1, 300, 1), t1.gcp(1.0, 100)
        mx, cc, sp, h, gm = comm.allreduce_u64([mx, cc, sp, h, gm])
        out = dict(ins=P[idx], ins_counts=cnt, ins2=P[idx2], ins2_counts=cnt2, mx=mx, cc=cc, sp=sp, h=h, gm=gm, packed=np.array(packed), xs=np.array(xs))
        if wide:
            out.update(got_hi=got[0], got_lo=got[1], got_counts=got[2])
        else:
            out.update(got_keys=got[0], got_counts=got[1])
        np.savez(os.path.join(out_dir, "case_%02d.rank%d.npz" % (ci, rank)), **out)
        t1.free()
        t2.free()
    if rank == 0:
        print("cases:", len(cases), "| transport:", comm.transport, "| chunks:", C, "| xs:", xs)
    comm.barrier()
    comm.free()
    eng.close()


if __name__ == "__main__":
    main()
