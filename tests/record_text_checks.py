"""What tests/test_gpu_cvg_text.py and tests/test_gpu_gc_text.py check a text call with: (text, offsets) against the model's, and the
device form called over buffers with guard bytes behind them."""
import numpy as np


def assert_equal(got, want, what=""):
    (text, off), (wtext, woff) = got, want
    assert isinstance(text, bytes) and off.dtype == np.uint64 and off.shape == woff.shape, (what, off.dtype, off.shape, woff.shape)
    bad = np.nonzero(off != woff)[0]
    assert bad.size == 0, (what, bad[:5], off[bad[:5]], woff[bad[:5]])
    if text != wtext:
        a, b = np.frombuffer(text, np.uint8), np.frombuffer(wtext, np.uint8)
        at = int(np.nonzero(a != b)[0][0]) if a.size == b.size else min(a.size, b.size)
        raise AssertionError((what, len(text), len(wtext), at, text[max(at - 30, 0):at + 30], wtext[max(at - 30, 0):at + 30]))


def device_call(engine, text_device, b, st, ln, cap, shift=0, guard=64):
    """text_device(dev_bases, n, dev_rec_start, dev_rec_len, n_rec, dev_text, cap, dev_text_off): the device form of a text, a bound
    method (Table.record_cvg_text_device; Engine.record_gc_text_device with its k in front).  The bases go up `shift` bytes into their
    buffer, the text buffer is `cap` + `guard` bytes of 0xAB, the offsets' n_rec + 2 words of 0xCD.  Returns (total, text buffer, the
    n_rec + 1 offsets)."""
    m = st.size
    db = engine.alloc(b.size + 64)
    db.upload(b, offset=shift)
    dr = engine.alloc(16 * m)
    dr.upload(st)
    dr.upload(ln, offset=8 * m)
    fill = np.full(cap + guard, 0xAB, np.uint8)
    do = engine.alloc(fill.nbytes)
    do.upload(fill)
    off_fill = np.full(m + 2, 0xCDCDCDCDCDCDCDCD, np.uint64)
    df = engine.alloc(off_fill.nbytes)
    df.upload(off_fill)
    total = text_device(db.ptr + shift, b.size, dr.ptr, dr.ptr + 8 * m, m, do.ptr if cap else None, cap, df.ptr)
    engine.sync()
    out, off = do.download(np.uint8, fill.size), df.download(np.uint64, off_fill.size)
    db.free(); dr.free(); do.free(); df.free()
    assert off[-1] == 0xCDCDCDCDCDCDCDCD                            # n_rec + 1 offsets, not one more
    return total, out, off[:-1]
