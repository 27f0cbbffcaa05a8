"""pcs_cloud_mlp_infer (csrc/cloud_mlp_infer.hip) rejects what it does not cover with an error message,
before any GPU work: no pointer below is ever dereferenced."""
import ctypes

import pytest

from pcseg import _lib, engine

FAKE = 0x1000


def rec(cin, cout, use_batch=0, act=0):
    return engine._REC.pack(FAKE, cin, cin, cout, 0, FAKE, FAKE, FAKE, FAKE, 0, 0.0, 1e-5, use_batch, act, 0.0,
                            0, 0, 0, 0, 0, 0, 0.0, 0, 0, 0)


GOOD = [rec(64, 64), rec(64, 128), rec(128, 1024, act=2)]
B, N = 2, 300                                   # 3 tiles of 128 rows per cloud


def workspace(recs):
    n = ctypes.c_size_t(0)
    rc = _lib.load().pcs_cloud_mlp_infer_workspace(B, N, b''.join(recs), len(recs), ctypes.byref(n))
    return rc, n.value


def test_workspace_of_a_covered_stack():
    assert workspace(GOOD) == (0, B * 3 * 1024 * 4)
    assert workspace(GOOD[1:]) == (0, B * 3 * 1024 * 4)


@pytest.mark.parametrize('recs,short,word', [
    ([rec(64, 128, use_batch=1), rec(128, 1024)], 0, b'training mode'),
    ([rec(64, 132), rec(132, 1024)], 0, b'width 132'),
    ([rec(64, 128), rec(128, 130)], 0, b'width 130'),
    (GOOD[2:], 0, b'1 layers'),
    (GOOD[:1] + GOOD, 0, b'4 layers'),
    ([rec(64, 128, act=2), rec(128, 1024)], 0, b'activation'),
    (GOOD, 4, b'workspace'),
])
def test_rejected_before_any_gpu_work(recs, short, word):
    lib = _lib.load()
    rc = lib.pcs_cloud_mlp_infer(FAKE, 64, 64, B, N, b''.join(recs), len(recs), FAKE, FAKE, B * 3 * 1024 * 4 - short, None)
    assert rc != 0
    msg = lib.pcs_last_error()
    assert b'pcs_cloud_mlp_infer' in msg and word in msg, msg
    if not short:
        assert workspace(recs)[0] != 0
