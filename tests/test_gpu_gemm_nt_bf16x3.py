"""Split-bf16 wide GEMM for training (csrc/gemm_big_bf16x3.hip, pcs_gemm_nt_bf16x3; opt-in through
PCS_GEMM_BF16X3 / engine.set_train_gemm) against A . B^T + bias in float64 on the CPU, and the engine and
model paths that take it against the fp32 path and a float64 torch reference.  Kernel shapes: M around the
256-row tile (600: a partial last tile, three statistics partials), N around the 128-column tile, R one and
three K slabs.  Bound 1e-4 norm-relative (tests/test_gpu_rows_infer.py's): the three-term split sits near
4.5e-6, a dropped cross term near 2e-3.  Statistics: fp64 sums of the stored fp32 values, 1e-10."""
import ctypes

import pytest
import torch

import pcseg
from pcseg import _lib, engine
from pcseg.engine import KernelProbe, call, ptr, set_train_gemm, shared_mlp, stream_ptr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TOL = 1e-4
NEW, OLD = 'pcs::gemm_nt_bf16x3_kernel', 'pcs::gemm_nt_kernel'


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _launch(a, b, bias, c, stats):
    call('pcs_gemm_nt_bf16x3', ptr(a), a.stride(0), ptr(b), b.stride(0), a.shape[0], b.shape[0], a.shape[1],
         ptr(bias), ptr(c), c.stride(0), ptr(stats), stream_ptr(c.device))


def _check_stats(stats, c):
    c = c.double()
    s = stats.sum(-1)                                  # over the 256-row tiles
    assert bool(((s[0] - c.sum(0)).abs() <= 1e-10 * c.abs().sum(0)).all())
    assert bool(((s[1] - (c * c).sum(0)).abs() <= 1e-10 * (c * c).sum(0)).all())


@pytest.mark.parametrize('N', [4, 128, 132, 260])
@pytest.mark.parametrize('M', [1, 255, 257, 600])
def test_kernel_matches_fp64(M, N):
    g = torch.Generator().manual_seed(1000 * M + N)
    tiles = _lib.load().pcs_gemm_nt_row_tiles(M)
    for R in (32, 96):
        a, b, bias = torch.randn(M, R, generator=g), torch.randn(N, R, generator=g), torch.randn(N, generator=g)
        prod = a.double() @ b.double().T
        ad, bd, biasd = a.to(DEV), b.to(DEV), bias.to(DEV)
        for with_bias in (False, True):
            ref = prod + bias.double() if with_bias else prod
            for with_stats in (False, True):
                c = torch.full((M, N), float('nan'), device=DEV)
                stats = torch.full((2, N, tiles), float('nan'), dtype=torch.float64, device=DEV) if with_stats else None
                _launch(ad, bd, biasd if with_bias else None, c, stats)
                print(f'M={M} N={N} R={R} bias={with_bias} stats={with_stats}: rel {rel(c, ref):.3e}')
                assert torch.isfinite(c).all() and rel(c, ref) <= TOL
                if with_stats:
                    _check_stats(stats, c)


def test_kernel_on_column_blocks_of_wider_buffers():
    M, N, R = 257, 132, 96
    g = torch.Generator().manual_seed(7)
    a, b, bias = torch.randn(M, R, generator=g), torch.randn(N, R, generator=g), torch.randn(N, generator=g)
    abuf = torch.full((M, R + 12), float('nan'), device=DEV)
    bbuf = torch.full((N, R + 8), float('nan'), device=DEV)
    cbuf = torch.full((M, N + 16), -7.0, device=DEV)       # the sentinel
    abuf[:, 8:8 + R] = a.to(DEV)
    bbuf[:, 4:4 + R] = b.to(DEV)
    stats = torch.full((2, N, 2), float('nan'), dtype=torch.float64, device=DEV)
    _launch(abuf[:, 8:8 + R], bbuf[:, 4:4 + R], bias.to(DEV), cbuf[:, 12:12 + N], stats)
    c = cbuf[:, 12:12 + N]
    assert rel(c, a.double() @ b.double().T + bias.double()) <= TOL
    _check_stats(stats, c)
    assert bool((cbuf[:, :12] == -7.0).all()) and bool((cbuf[:, 12 + N:] == -7.0).all())


# ------------------------------------------------------------------ engine path
ROWS, CH = 65536, 256          # the smallest gemm_nt-regime shape for the forward and the data gradient


def _layer_inputs():
    g = torch.Generator().manual_seed(11)
    x, W = torch.randn(ROWS, CH, generator=g), torch.randn(CH, CH, generator=g) / CH ** 0.5
    gamma, beta = torch.rand(CH, generator=g) + 0.5, 0.1 * torch.randn(CH, generator=g)
    return x, W, gamma, beta, torch.randn(ROWS, CH, generator=g)       # .., the output gradient


def _layer_fp64(inputs, positive):
    """The layer and its backward in float64 on the CPU: (out, dX, dW, dgamma, dbeta).  The LeakyReLU branch
    is taken from `positive`, the GPU run's own sign decisions, as the project's fp64 truth does
    (tests/fp64_check.py): ~30 of the 16.8 M signs differ at 4e-6, which alone moves dX and dW by 1.5e-3."""
    *leaves, gout = (t.double() for t in inputs)
    for t in leaves:
        t.requires_grad_()
    z = leaves[0] @ leaves[1].T
    y = (z - z.mean(0)) / (z.var(0, unbiased=False) + 1e-5).sqrt() * leaves[2] + leaves[3]
    out = torch.where(positive, y, 0.2 * y)
    out.backward(gout)
    return (out.detach(), *(t.grad for t in leaves))


def _run_layer(inputs, gemm):
    x, W, gamma, beta, gout = (t.to(DEV) for t in inputs)
    conv = torch.nn.Conv1d(CH, CH, 1, bias=False).to(DEV)
    bn = torch.nn.BatchNorm1d(CH).to(DEV).train()
    with torch.no_grad():
        conv.weight.copy_(W.view(CH, CH, 1))
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    x.requires_grad_()
    with KernelProbe() as kp:
        out = shared_mlp(x, CH, [conv], [bn], 'lrelu', 0.2, gemm=gemm)
        out.backward(gout)
        torch.cuda.synchronize()
    names = [r[0] for r in kp.records()]
    return (out.detach(), x.grad, conv.weight.grad.view(CH, CH), bn.weight.grad, bn.bias.grad), names


def test_engine_layer_takes_the_kernel_under_the_flag():
    inputs = _layer_inputs()
    got, names = _run_layer(inputs, 'bf16x3')
    base, base_names = _run_layer(inputs, 'fp32')
    errs = [rel(a, b) for a, b in zip(got, _layer_fp64(inputs, got[0].cpu() > 0))]
    print('out dX dW dgamma dbeta vs fp64', errs, 'out vs fp32 path', rel(got[0], base[0]))
    assert max(errs) <= 1e-3
    assert rel(got[0], base[0]) <= TOL
    assert names.count(NEW + '<true>') == 1 and names.count(NEW + '<false>') == 1       # forward, data gradient
    assert not any(n.startswith(OLD) for n in names)
    assert sum(n.startswith(OLD) for n in base_names) == 2 and not any(n.startswith(NEW) for n in base_names)


def test_dgcnn_training_step_dispatch():
    torch.manual_seed(5)
    model = pcseg.DGCNNWithColor(13, k=16).to(DEV).train()       # the smallest k the kNN kernels are built for
    x = torch.randn(16, 6, 4096).to(DEV)
    with pytest.raises(ValueError):
        set_train_gemm(model, 'fp16')
    logits, names = {}, {}
    for mode in ('fp32', 'bf16x3'):
        set_train_gemm(model, mode)
        model.zero_grad()
        torch.manual_seed(9)                    # the fused dropouts' mask seeds
        with KernelProbe() as kp:
            out = model(x)[0]
            out.square().mean().backward()
            torch.cuda.synchronize()
        logits[mode], names[mode] = out.detach(), [r[0] for r in kp.records()]
    print('logits bf16x3 vs fp32', rel(logits['bf16x3'], logits['fp32']))
    new = {k: (v.count(NEW + '<true>'), v.count(NEW + '<false>')) for k, v in names.items()}
    old = {k: sum(n.startswith(OLD) for n in v) for k, v in names.items()}
    assert new == {'fp32': (0, 0), 'bf16x3': (3, 3)} and old == {'fp32': 6, 'bf16x3': 0}     # conv5-7, both ways
    assert torch.isfinite(logits['bf16x3']).all() and rel(logits['bf16x3'], logits['fp32']) <= TOL


def test_argument_checks():
    lib = _lib.load()
    fake = 0x1000                       # never dereferenced: every call fails its checks first
    # (A, B, C, N, R, ldc): R % 32, N % 4, ldc < N, a misaligned pointer
    for A, B, C, N, R, ldc in ((fake, fake, fake, 8, 48, 8), (fake, fake, fake, 6, 32, 8), (fake, fake, fake, 8, 32, 4),
                               (fake + 4, fake, fake, 8, 32, 8), (fake, fake, fake + 8, 8, 32, 8)):
        assert lib.pcs_gemm_nt_bf16x3(A, 64, B, 64, 16, N, R, None, C, ldc, None, None) != 0
        assert b'pcs_gemm_nt_bf16x3' in lib.pcs_last_error()

    def workspace(bwd_fuse):
        rec = engine._REC.pack(16, 64, 64, 64, 0, 0, 0, 16, 16, 0, 0.0, 1e-5, 1, 0, 0.0, 16, 16, 0, 0, 0, 0, 0.0, 0,
                               bwd_fuse, 0)
        return lib.pcs_mlp_workspace(1024, 64, 64, rec, 1, 0, 1, ctypes.byref(ctypes.c_size_t(0)))
    assert workspace(engine.GEMM_BF16X3) == 0 and workspace(engine.GEMM_BF16X3 | engine.BWD_FUSE['all']) == 0
    assert workspace(engine.GEMM_BF16X3 | 3) != 0 and b'bwd_fuse' in lib.pcs_last_error()
    with pytest.raises(ValueError):
        shared_mlp(torch.zeros(8, 4, device=DEV), 4, [], [], gemm='fp16')
