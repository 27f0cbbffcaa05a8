"""Split-bf16 wide weight gradient (csrc/wgrad_bf16x3.hip, pcs_wgrad_bf16x3; opt-in through PCS_WGRAD_BF16X3 /
engine.set_train_gemm(model, 'bf16x3+wgrad')) against dW0 + X^T . Y in float64 on the CPU, and the engine and
model paths that take it against the 'bf16x3' path.  Bound 1e-4 norm-relative (tests/test_gpu_gemm_nt_bf16x3.py's):
the three-term split sits near 4.5e-6, a dropped cross term near 2e-3."""
import ctypes

import pytest
import torch

import pcseg
from pcseg import _lib, engine
from pcseg.engine import KernelProbe, call, ptr, set_train_gemm, stream_ptr
from test_gpu_gemm_nt_bf16x3 import _layer_fp64, _layer_inputs, _run_layer

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TOL = 1e-4
NEW, OLD = 'pcs::wgrad_bf16x3_kernel', ('pcs::wgrad_kernel', 'pcs::wgrad_nt_kernel')


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _launch(x, y, dW):
    """dW += x^T . y on the kernel; returns the number of row splits (from the workspace size)."""
    M, N, K = x.shape[0], x.shape[1], y.shape[1]
    n = ctypes.c_size_t(0)
    call('pcs_wgrad_bf16x3_workspace', N, K, M, ctypes.byref(n))
    ws = torch.empty(n.value, dtype=torch.uint8, device=DEV)
    call('pcs_wgrad_bf16x3', ptr(x), x.stride(0), ptr(y), y.stride(0), M, N, K, ptr(dW), ptr(ws), n.value,
         stream_ptr(dW.device))
    return (n.value - 256) // (4 * N * K)


@pytest.mark.parametrize('K', [4, 132])
@pytest.mark.parametrize('N', [4, 128, 132, 260])
@pytest.mark.parametrize('M', [1, 31, 33, 257, 1000])
def test_kernel_matches_fp64(M, N, K):
    g = torch.Generator().manual_seed(100000 * M + 1000 * N + K)
    x, y, dW0 = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    dW = dW0.to(DEV)
    splits = _launch(x.to(DEV), y.to(DEV), dW)
    err = rel(dW, dW0.double() + x.double().T @ y.double())
    print(f'M={M} N={N} K={K} splits={splits}: rel {err:.3e}')
    assert M != 1000 or splits > 1                         # 1000 rows: splits of 32 rows, the last of 8
    assert torch.isfinite(dW).all() and err <= TOL


def test_identical_calls_are_bitwise_identical():
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(1000, 260, generator=g).to(DEV), torch.randn(1000, 132, generator=g).to(DEV)
    a = torch.randn(260, 132, generator=g).to(DEV)
    b = a.clone()
    assert _launch(x, y, a) > 1 and _launch(x, y, b) > 1
    assert torch.equal(a, b)


def test_kernel_on_column_blocks_of_wider_buffers():
    M, N, K = 257, 132, 96
    g = torch.Generator().manual_seed(7)
    x, y, dW0 = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    xbuf = torch.full((M + 1, N + 12), float('nan'), device=DEV)       # a NaN row past M as well
    ybuf = torch.full((M + 1, K + 8), float('nan'), device=DEV)
    xbuf[:M, 8:8 + N] = x.to(DEV)
    ybuf[:M, 4:4 + K] = y.to(DEV)
    dW = dW0.to(DEV)
    _launch(xbuf[:M, 8:8 + N], ybuf[:M, 4:4 + K], dW)
    assert torch.isfinite(dW).all() and rel(dW, dW0.double() + x.double().T @ y.double()) <= TOL


def test_engine_layer_takes_the_kernel_under_the_flag():
    inputs = _layer_inputs()
    got, names = _run_layer(inputs, 'bf16x3+wgrad')
    base, base_names = _run_layer(inputs, 'bf16x3')
    errs = [rel(a, b) for a, b in zip(got, _layer_fp64(inputs, got[0].cpu() > 0))]
    print('out dX dW dgamma dbeta vs fp64', errs, 'dW vs bf16x3 path', rel(got[2], base[2]))
    assert names.count(NEW) == 1 and not any(n.startswith(OLD) for n in names)
    assert NEW not in base_names and sum(n.startswith(OLD) for n in base_names) == 1
    assert all(torch.equal(got[i], base[i]) for i in (0, 1, 3, 4))     # only the product's arithmetic differs
    assert rel(got[2], base[2]) <= TOL
    assert max(errs) <= 1e-3


def test_dgcnn_training_step_dispatch():
    torch.manual_seed(5)
    model = pcseg.DGCNNWithColor(13, k=16).to(DEV).train()       # the smallest k the kNN kernels are built for
    x = torch.randn(16, 6, 4096).to(DEV)
    with pytest.raises(ValueError):
        set_train_gemm(model, 'nope')
    logits, names, grads = {}, {}, {}
    for mode in ('bf16x3', 'bf16x3+wgrad'):
        set_train_gemm(model, mode)
        model.zero_grad()
        torch.manual_seed(9)                    # the fused dropouts' mask seeds
        with KernelProbe() as kp:
            out = model(x)[0]
            out.square().mean().backward()
            torch.cuda.synchronize()
        logits[mode], names[mode] = out.detach(), [r[0] for r in kp.records()]
        grads[mode] = [c[0].weight.grad.clone() for c in (model.conv5, model.conv6, model.conv7)]
    new = {k: v.count(NEW) for k, v in names.items()}
    old = {k: sum(n.startswith(OLD) for n in v) for k, v in names.items()}
    errs = [rel(a, b) for a, b in zip(grads['bf16x3+wgrad'], grads['bf16x3'])]
    print('conv5-7 dW vs bf16x3', errs, 'old weight-gradient launches', old)
    assert new == {'bf16x3': 0, 'bf16x3+wgrad': 3} and old['bf16x3+wgrad'] == old['bf16x3'] - 3
    assert torch.equal(logits['bf16x3+wgrad'], logits['bf16x3'])
    assert max(errs) <= TOL


def test_argument_checks():
    lib = _lib.load()
    fake, big = 0x1000, 1 << 30         # never dereferenced: every call fails its checks first
    # (X, N, K, ldx, workspace bytes): N % 4, K % 4, ldx < N, a misaligned X, a too-small workspace
    for X, N, K, ldx, nws in ((fake, 6, 8, 64, big), (fake, 8, 6, 64, big), (fake, 8, 8, 4, big),
                              (fake + 4, 8, 8, 64, big), (fake, 8, 8, 64, 16)):
        assert lib.pcs_wgrad_bf16x3(X, ldx, fake, 64, 16, N, K, fake, fake, nws, None) != 0
        assert b'pcs_wgrad_bf16x3' in lib.pcs_last_error()

    def workspace(bwd_fuse):
        rec = engine._REC.pack(16, 64, 64, 64, 0, 0, 0, 16, 16, 0, 0.0, 1e-5, 1, 0, 0.0, 16, 16, 0, 0, 0, 0, 0.0, 0,
                               bwd_fuse, 0)
        return lib.pcs_mlp_workspace(1024, 64, 64, rec, 1, 0, 1, ctypes.byref(ctypes.c_size_t(0)))
    assert workspace(engine.WGRAD_BF16X3) == 0 and workspace(engine.WGRAD_BF16X3 | engine.GEMM_BF16X3) == 0
    assert workspace(0x400) != 0 and b'bwd_fuse' in lib.pcs_last_error()
