"""pcs_fp_head_infer (csrc/fp_head_infer.hip) rejects what it does not cover with an error message, before
any GPU work: no pointer below is ever dereferenced."""
import ctypes

import pytest

from pcseg import _lib, engine

FAKE = 0x1000
B, N = 3, 300


def rec(cin, cout, use_batch=0, act=0, bn=FAKE, W=FAKE):
    return engine._REC.pack(W, cin, cin, cout, 0, bn, bn, bn, bn, 0, 0.0, 1e-5, use_batch, act, 0.0,
                            0, 0, 0, 0, 0, 0, 0.0, 0, 0, 0)


def tail(d1=0, nl=4, w=128, classes=13):
    return [rec(d1 + 128 if l == 0 else w, w) for l in range(nl)] + [rec(w, classes, act=2, bn=0)]


def workspace(recs, M=16, d1=0, d2=128):
    n = ctypes.c_size_t(7)
    rc = _lib.load().pcs_fp_head_infer_workspace(B, N, M, d1, d2, b''.join(recs), len(recs), ctypes.byref(n))
    return rc, n.value


@pytest.mark.parametrize('d1,nl', [(0, 4), (0, 3), (32, 4), (4, 1)])      # PointNetpp, PointNetppMSG, PointNeXt
def test_covered_tails_need_no_workspace(d1, nl):
    assert workspace(tail(d1, nl), d1=d1) == (0, 0)
    assert workspace(tail(d1, nl, classes=32), M=3, d1=d1) == (0, 0)


@pytest.mark.parametrize('recs,kw,ptrs,word', [
    (tail(w=132), {}, {}, b'width 132'),
    (tail(nl=0), {}, {}, b'1 records'),
    (tail(nl=5), {}, {}, b'6 records'),
    (tail(), {'d2': 64}, {}, b'D2 64'),
    (tail(36), {'d1': 36}, {}, b'D1 36'),
    (tail(6), {'d1': 6}, {}, b'D1 6'),
    (tail(classes=0), {}, {}, b'classes 0'),
    (tail(classes=33), {}, {}, b'classes 33'),
    (tail(), {'M': 2}, {}, b'M 2'),
    ([rec(128, 128, use_batch=1)] + tail()[1:], {}, {}, b'training mode'),
    ([rec(128, 128, W=FAKE + 4)] + tail()[1:], {}, {}, b'16-B aligned'),
    ([rec(128, 128, W=0)] + tail()[1:], {}, {}, b'null pointer'),
    (tail(), {}, {'f2': None}, b'null pointer'),
    (tail(), {}, {'idx': None}, b'null pointer'),
    (tail(), {}, {'out': None}, b'null pointer'),
    (tail(32), {'d1': 32}, {'f1': None}, b'null pointer'),
    (tail(32), {'d1': 32}, {'f1': FAKE + 4}, b'16-B aligned'),
])
def test_rejected_before_any_gpu_work(recs, kw, ptrs, word):
    lib = _lib.load()
    M, d1, d2 = kw.get('M', 16), kw.get('d1', 0), kw.get('d2', 128)
    p = {'f1': FAKE if d1 else None, 'f2': FAKE, 'idx': FAKE, 'dist': FAKE, 'out': FAKE, **ptrs}
    rc = lib.pcs_fp_head_infer(p['f1'], 32, d1, p['f2'], d2, p['idx'], p['dist'], B, N, M, b''.join(recs), len(recs),
                               p['out'], 32, None, None)
    assert rc != 0
    msg = lib.pcs_last_error()
    assert b'pcs_fp_head_infer' in msg and word in msg, msg
    if not ptrs:
        assert workspace(recs, M, d1, d2)[0] != 0
