"""pcs_point_head_infer (csrc/point_head_infer.hip) rejects what it does not cover with an error message,
before any GPU work: no pointer below is ever dereferenced."""
import ctypes

import pytest

from pcseg import _lib, engine

FAKE = 0x1000
KG = 1024


def rec(cin, cout, use_batch=0, act=0, bn=FAKE):
    return engine._REC.pack(FAKE, cin, cin, cout, 0, bn, bn, bn, bn, 0, 0.0, 1e-5, use_batch, act, 0.0,
                            0, 0, 0, 0, 0, 0, 0.0, 0, 0, 0)


def head(kp=64, w=(512, 256, 128), classes=14):
    return [rec(KG + kp, w[0]), rec(w[0], w[1]), rec(w[1], w[2]), rec(w[2], classes, act=2, bn=0)]


B, N = 3, 300
WS = B * 512 * 4                                # the per-cloud biases c[b][512]


def workspace(recs):
    n = ctypes.c_size_t(0)
    rc = _lib.load().pcs_point_head_infer_workspace(B, N, KG, b''.join(recs), len(recs), ctypes.byref(n))
    return rc, n.value


def test_workspace_of_a_covered_head():
    assert workspace(head()) == (0, WS)
    assert workspace(head(kp=128, classes=32)) == (0, WS)
    assert workspace(head(kp=4, classes=1)) == (0, WS)


@pytest.mark.parametrize('recs,short,word', [
    ([rec(KG + 64, 512, use_batch=1)] + head()[1:], 0, b'training mode'),
    (head(w=(512, 130, 128)), 0, b'width 130'),
    (head()[3:], 0, b'1 layers'),
    (head(classes=33), 0, b'classes 33'),
    (head(kp=132), 0, b'kp 132'),
    (head()[:3] + [rec(128, 14, act=2)], 0, b'BatchNorm'),
    (head(), 4, b'workspace'),
])
def test_rejected_before_any_gpu_work(recs, short, word):
    lib = _lib.load()
    rc = lib.pcs_point_head_infer(FAKE, 64, FAKE, KG, KG, B, N, b''.join(recs), len(recs), 1, FAKE, 16, FAKE,
                                  WS - short, None)
    assert rc != 0
    msg = lib.pcs_last_error()
    assert b'pcs_point_head_infer' in msg and word in msg, msg
    if not short:
        assert workspace(recs)[0] != 0
