"""Eval-mode EdgeConv (csrc/edgeconv_infer.hip, pcs_edgeconv_infer) against the reference layer
(models/dgcnn/dgcnn.py:24-77 under eval()) written out in float64 on the CPU with the same index
table: gather [x_j - x_i ; x_i], 1x1 conv, BN on the running statistics, LeakyReLU(0.2), max over k.
Norm-relative bound: the EdgeConv TOL of test_gpu_edgeconv.py (same decomposition, fp32 MFMA).

B = 3 clouds of N = 173 points (M = 519): a ragged 128-row GEMM tile, a ragged points-per-wave tail
and clouds aligned to nothing; k = 20 and 5 are no multiple of the gather batch of 8 (5 < one batch)."""
import pytest
import torch
import torch.nn.functional as F

import pcseg
from pcseg import _lib
from pcseg.engine import edgeconv_fused_ok, edgeconv_infer, edgeconv_infer_ok, storage_alias

DEV = 'cuda'
TOL = 1e-4
B, N = 3, 173
NEG, ZERO = [1, 6, 33, 62], [2, 40]          # channels with gamma < 0 / gamma == 0


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _case(C, Cout, k, seed):
    """x (B, N, C), idx (B, N, k) int32, an eval-mode pcseg.EdgeConv with non-trivial BN state, and
    the fp64 reference: out (B*N, Cout), the edge pre-activations z (B, N, k, Cout) and BN's (s, t, beta)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, C, generator=g)
    idx = torch.randint(0, N, (B, N, k), generator=g, dtype=torch.int32)
    m = pcseg.EdgeConv(C, Cout, k).eval()
    conv, bn = m.conv[0], m.conv[1]
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / (2 * C) ** 0.5)
        bn.weight.copy_(torch.rand(Cout, generator=g) + 0.5)
        bn.weight[NEG] *= -1
        bn.weight[ZERO] = 0
        bn.bias.copy_(torch.randn(Cout, generator=g))
        bn.running_mean.copy_(0.5 * torch.randn(Cout, generator=g))
        bn.running_var.copy_(torch.rand(Cout, generator=g) + 0.3)
    xd = x.double()
    nb = xd[torch.arange(B)[:, None, None], idx.long()]                       # (B, N, k, C)
    ctr = xd.unsqueeze(2).expand_as(nb)
    z = torch.cat([nb - ctr, ctr], -1) @ conv.weight.detach().double().flatten(1).T
    y = (z - bn.running_mean.double()) / (bn.running_var.double() + bn.eps).sqrt() * bn.weight.double() + bn.bias.double()
    s = bn.weight.detach().double() / (bn.running_var.double() + bn.eps).sqrt()
    coef = (s, bn.bias.detach().double() - bn.running_mean.double() * s, bn.bias.detach().clone())
    return x, idx, m, F.leaky_relu(y, 0.2).detach().max(2).values.reshape(B * N, Cout), z, coef


@pytest.mark.gpu
@pytest.mark.parametrize('k', [20, 5])
@pytest.mark.parametrize('C,Cout', [(3, 64), (64, 64), (64, 128)])
def test_edgeconv_infer_matches_fp64(C, Cout, k):
    x, idx, m, ref, z, (s, t, beta) = _case(C, Cout, k, seed=C + Cout + k)
    m = m.to(DEV)
    out = edgeconv_infer(x.reshape(B * N, C).to(DEV), C, idx.to(DEV), m.conv[0], m.conv[1], 0.2).cpu()
    assert out.shape == ref.shape and torch.isfinite(out).all()
    assert rel(out, ref) < TOL
    # s < 0: the pooled edge is the one with the smallest z (alone, so the other channels cannot hide it)
    lo = F.leaky_relu(z.min(2).values.reshape(B * N, Cout) * s + t, 0.2)
    assert rel(out[:, NEG], lo[:, NEG]) < TOL
    # gamma == 0: act(beta) exactly, whatever the neighbours are
    assert torch.equal(out[:, ZERO], F.leaky_relu(beta[ZERO], 0.2).expand(B * N, -1))


@pytest.mark.gpu
def test_edgeconv_infer_strided_input_second_output_weight_at_storage_end():
    C = Cout = 64
    x, idx, m, ref, _, _ = _case(C, Cout, 20, seed=9)
    m = m.to(DEV)
    conv = m.conv[0]
    n = conv.weight.numel()
    store = torch.full((256 + n,), float('nan'), device=DEV)      # the weight ends where its storage ends
    store[256:].copy_(conv.weight.detach().flatten())
    conv.weight = torch.nn.Parameter(store[256:].view_as(conv.weight))
    wide = torch.full((B * N, 192), float('nan'), device=DEV)
    xin = storage_alias(wide, 64, C)                              # ldx = 192
    xin.copy_(x.reshape(B * N, C))
    H = torch.full((B * N, 1408), float('nan'), device=DEV)
    blk = storage_alias(H, 192, Cout)
    out = edgeconv_infer(xin, C, idx.to(DEV), conv, m.conv[1], 0.2, also=blk)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and rel(out, ref) < TOL
    assert torch.equal(blk, out)
    assert torch.isnan(H[:, :192]).all() and torch.isnan(H[:, 192 + Cout:]).all()
    assert torch.isnan(wide[:, :64]).all() and torch.isnan(wide[:, 128:]).all() and torch.isnan(store[:256]).all()


@pytest.mark.gpu
def test_edgeconv_module_dispatches_eval_no_grad_to_infer_kernels():
    x, idx, m, ref, _, _ = _case(64, 64, 20, seed=4)
    m = m.to(DEV)
    conv, bn = m.conv[0], m.conv[1]
    assert edgeconv_infer_ok(conv, bn, 64) and not edgeconv_fused_ok(conv, bn, 64)
    state = [v.clone() for v in (bn.running_mean, bn.running_var, bn.num_batches_tracked)]
    xc = x.transpose(1, 2).contiguous().to(DEV)                  # the module's (B, C, N) layout
    with torch.no_grad(), pcseg.replay(pcseg.Replay(knn_idx=[idx])):
        o = m(xc)
    with pcseg.replay(pcseg.Replay(knn_idx=[idx])):
        o_grad = m(xc.requires_grad_(True))                       # eval-mode BN with a backward: materialised edges
    assert not o.requires_grad and o_grad.requires_grad
    assert rel(o.transpose(1, 2).reshape(B * N, 64), ref) < TOL
    assert rel(o, o_grad.detach()) < TOL
    for a, b in zip(state, (bn.running_mean, bn.running_var, bn.num_batches_tracked)):
        assert torch.equal(a, b)
    assert not edgeconv_infer_ok(conv, m.train().conv[1], 64)


def test_edgeconv_infer_argument_checks_without_gpu():
    lib = _lib.load()
    fake = 0x1000                       # never dereferenced: every call fails its checks first
    for n_, k, cout, ix in ((8, 9, 64, fake), (8, 4, 6, fake), (8, 4, 64, None)):
        rc = lib.pcs_edgeconv_infer(fake, 64, 64, ix, 1, n_, k, fake, cout, fake, fake, fake, fake, 1e-5, 0.2,
                                    fake, fake, fake, None, 0, None)
        assert rc != 0
        assert b'pcs_edgeconv_infer' in lib.pcs_last_error()
