"""Pins tests/jf_order_model_wide.py to the host .jf writer for two-word k-mers (katgpu_jf_write_records_wide): the model's bytes are
the file's bytes, and the reference's own reader (file_header + binary_reader + multi-word mer_dna, oracle/_ref/jf_ref jfread) decodes
the records the model says the file holds, at the positions it says.  The model is the yardstick of tests/test_gpu_jf_dump_wide.py."""
import numpy as np
import pytest

import kat_amd
from tests import jf_order_model_wide as model
from tests import refcalls

U64 = np.uint64
N = 3000


def make_records(k):
    rng = np.random.default_rng(k)
    hi_bits = 2 * k - 64
    hi = rng.integers(0, 1 << hi_bits, size=N, dtype=U64)
    lo = rng.integers(0, 1 << 64, size=N, dtype=U64)
    # twins that differ only in hi, twins that differ only in lo (in its top bit: a signed compare would turn them round), the all-ones key
    hi = np.concatenate([hi, hi[:40] ^ U64(1), hi[40:80], [U64((1 << hi_bits) - 1)]]).astype(U64)
    lo = np.concatenate([lo, lo[:40], lo[40:80] ^ U64(1 << 63), [U64(2**64 - 1)]]).astype(U64)
    _, first = np.unique(np.stack([hi, lo], 1), axis=0, return_index=True)
    keep = np.sort(first)
    hi, lo = hi[keep], lo[keep]
    assert hi.size >= N + 80
    counts = rng.integers(1, 1 << 20, size=hi.size, dtype=U64)
    counts[:4] = np.array([2**32 - 1, 2**32, 2**32 + 5, 2**40], U64)
    counts[-1] = U64(2**32 - 2)
    return hi, lo, counts


@pytest.fixture(scope="module", params=[33, 36, 47, 63])
def written(request, tmp_path_factory):
    k = request.param
    hi, lo, counts = make_records(k)
    path = str(tmp_path_factory.mktemp("jfw") / ("m%d.jf" % k))
    kat_amd.jf_write_records_wide(path, k, bool(k & 1), hi, lo, counts)
    return k, hi, lo, counts, path


def test_model_equals_host_writer(written):
    k, hi, lo, counts, path = written
    hdr, _, body = model.split(path)
    r, cols = model.matrix(hdr)
    assert hdr["key_len"] == 2 * k and hdr["counter_len"] == 4 and hdr["canonical"] == bool(k & 1) and cols.size == 2 * k
    want, pos, shi, slo = model.record_bytes(k, hi, lo, counts, cols, r)
    assert len(body) == hi.size * ((2 * k + 7) // 8 + 4)
    assert body == want
    # equal positions occur, and inside such runs the order is by hi before lo: the tie order is part of what is pinned
    same = np.diff(pos) == 0
    assert r < 2 * k and same.any()
    assert (same & (shi[1:] > shi[:-1]) & (slo[1:] < slo[:-1])).any()
    if k <= 36:                                             # few hi bits: runs whose order only lo decides
        assert (same & (shi[1:] == shi[:-1])).any()
    # the cut by position the device entry point is checked against
    cuts = [0, (1 << r) // 3, (1 << r) - 2, 1 << r]
    assert b"".join(model.record_bytes(k, hi, lo, counts, cols, r, a, b)[0] for a, b in zip(cuts, cuts[1:])) == want


def test_reference_reader_decodes_the_model(written):
    k, hi, lo, counts, path = written
    if not refcalls.built(refcalls.JF_REF):
        args = ["jfread", path]
        if refcalls._key(refcalls.JF_REF, args, None, refcalls._subs(args)) not in refcalls._load():
            pytest.skip("oracle/_ref/jf_ref is not built and holds no recorded answer for this file")
    from tests.test_oracle_vs_reference import parse_jfread
    rc, out = refcalls.run(refcalls.JF_REF, ["jfread", path], rebuild=lambda: refcalls.jfread_text(path))
    assert rc == 0
    h, recs = parse_jfread(out)
    hdr, _, _ = model.split(path)
    r, cols = model.matrix(hdr)
    _, pos, shi, slo = model.record_bytes(k, hi, lo, counts, cols, r)
    assert h["key_len"] == str(2 * k) and len(recs) == hi.size
    order = np.lexsort((lo, hi, model.positions(hi, lo, cols, r)))
    sat = np.minimum(counts[order], U64(0xFFFFFFFF))
    for i, (mer, count, p) in enumerate(recs):
        word = (int(shi[i]) << 64) | int(slo[i])
        assert mer == "".join("ACGT"[(word >> (2 * (k - 1 - j))) & 3] for j in range(k)), i
        assert (count, p) == (int(sat[i]), int(pos[i])), i
