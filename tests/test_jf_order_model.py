"""Pins tests/jf_order_model.py to the host .jf writer (katgpu_jf_write_records): the model's bytes are the file's bytes."""
import numpy as np
import pytest

import kat_amd
from tests import jf_order_model as model


@pytest.mark.parametrize("k", [5, 13, 21, 27, 32])
@pytest.mark.parametrize("n", [0, 1, 2, 1000])
def test_model_equals_host_writer(tmp_path, k, n):
    rng = np.random.default_rng(1000 * k + n)
    space = 1 << (2 * k)
    if space <= 1 << 20:
        keys = rng.permutation(space)[:n].astype(np.uint64)
    else:
        keys = np.unique(rng.integers(0, space, size=2 * n + 8, dtype=np.uint64, endpoint=False))
        keys = rng.permutation(keys)[:n]
    if k == 32 and n:
        keys[0] = np.uint64(2**64 - 1)                     # the all-ones 32-mer
    assert np.unique(keys).size == n
    counts = rng.integers(1, 1 << 20, size=n, dtype=np.uint64)
    if n:
        counts[-1] = np.uint64(2**32 + 5)                  # saturates
    path = str(tmp_path / "m.jf")
    kat_amd.jf_write_records(path, k, bool(n & 1), keys, counts)
    hdr, _, body = model.split(path)
    r, cols = model.matrix(hdr)
    assert hdr["key_len"] == 2 * k and hdr["counter_len"] == 4 and hdr["canonical"] == bool(n & 1)
    want, pos = model.record_bytes(k, keys, counts, cols, r)
    assert len(body) == n * ((2 * k + 7) // 8 + 4)
    assert body == want
    if n == 1000 and k > 5:
        assert r < 2 * k and (np.diff(pos) == 0).any()     # equal positions occur: the tie order is part of what is pinned
