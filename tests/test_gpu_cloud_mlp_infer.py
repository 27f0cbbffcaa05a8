"""Fused eval-mode PointNet stack + per-cloud max-pool (csrc/cloud_mlp_infer.hip, pcs_cloud_mlp_infer)
against the stack written out in float64 on the CPU: 1x1 conv with bias, BN on the running statistics,
ReLU (the last layer: ReLU or none), max over each cloud's N points.

Bound 5e-5 norm-relative: the dropped lo*lo term and the split residual are each <= 2^-16 relative per
product, over three layers ~ 4.6e-5; a kernel that loses a hi*lo term sits near 2^-9 ~ 2e-3.
Measured on an MI355X (B, N, kin/ld, widths, last act):
  (1, 100, 9/12, 64-128-1024, relu) 3.0e-06   (3, 256, 64, 64-128-1024, relu) 2.7e-06
  (2, 257, 64, 128-1024, none)      2.4e-06   (2, 600, 64, 128-128, none)     2.3e-06"""
import pytest
import torch

import pcseg
from pcseg import engine
from pcseg.engine import cloud_mlp_infer, cloud_mlp_infer_ok, set_eval_fuse

DEV = 'cuda'
PROBE = 'pcs::cloud_mlp_infer_kernel'


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def stack_fp64(x, convs, bns, acts):
    """x (B, N, kin) -> (B, C_last): conv, eval BN from the running statistics, ReLU or none, max over N."""
    x = x.double()
    for conv, bn, act in zip(convs, bns, acts):
        z = x @ conv.weight.detach().double().flatten(1).T + conv.bias.detach().double()
        x = ((z - bn.running_mean.double()) / (bn.running_var.double() + bn.eps).sqrt() * bn.weight.detach().double()
             + bn.bias.detach().double())
        x = torch.relu(x) if act == 'relu' else x
    return x.max(1).values


@pytest.mark.gpu
@pytest.mark.parametrize('B,N,kin,ld,widths,last', [(1, 100, 9, 12, (64, 128, 1024), 'relu'),
                                                    (3, 256, 64, 64, (64, 128, 1024), 'relu'),
                                                    (2, 257, 64, 64, (128, 1024), 'none'),
                                                    (2, 600, 64, 64, (128, 128), 'none')])
def test_cloud_mlp_infer_matches_fp64(B, N, kin, ld, widths, last):
    g = torch.Generator().manual_seed(N + kin)
    convs, bns, cin = [], [], kin
    for n in widths:
        conv, bn = torch.nn.Conv1d(cin, n, 1), torch.nn.BatchNorm1d(n).eval()
        with torch.no_grad():
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / cin ** 0.5)
            conv.bias.copy_(0.1 * torch.randn(n, generator=g))
            bn.weight.copy_(torch.rand(n, generator=g) + 0.5)
            bn.weight[1::7] *= -1                       # gamma < 0
            bn.weight[2::9] = 0                         # gamma == 0: the channel is beta
            bn.bias.copy_(torch.randn(n, generator=g))  # a zero input row would win where b' is the largest
            bn.running_mean.copy_(0.5 * torch.randn(n, generator=g))
            bn.running_var.copy_(torch.rand(n, generator=g) + 0.3)
        convs.append(conv), bns.append(bn)
        cin = n
    acts = ('relu',) * (len(widths) - 1) + (last,)
    x = torch.randn(B, N, kin, generator=g)
    ref = stack_fp64(x, convs, bns, acts)
    rows = torch.full((B * N, ld), 7.0)                 # columns kin .. ld are not channels
    rows[:, :kin] = x.reshape(B * N, kin)
    convs, bns = [c.to(DEV) for c in convs], [b.to(DEV) for b in bns]
    assert cloud_mlp_infer_ok(convs, bns, kin, acts)
    out = cloud_mlp_infer(rows.to(DEV), kin, B, N, convs, bns, acts)
    again = cloud_mlp_infer(rows.to(DEV), kin, B, N, convs, bns, acts)
    print('rel vs fp64', rel(out, ref))
    assert out.shape == ref.shape and torch.isfinite(out).all()
    assert rel(out, ref) <= 5e-5
    assert torch.equal(out, again)


@pytest.mark.gpu
def test_pointnet_takes_the_fused_path_only_in_eval_without_grad():
    torch.manual_seed(3)
    model = pcseg.PointNetSeg(14).to(DEV).eval()
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
    x = torch.rand(2, 300, 9, device=DEV)

    def run(fuse, grad=False, train=False):
        set_eval_fuse(model, fuse)
        model.train(train)
        with torch.set_grad_enabled(grad), engine.KernelProbe() as kp:
            y = model(x)
        model.eval()
        return y.detach(), sum(r[0] == PROBE for r in kp.records())

    off, n_off = run(False)
    on, n_on = run(True)
    assert (n_off, n_on) == (0, 2)                      # STN + encoder
    assert run(True, grad=True)[1] == 0 and run(True, train=True)[1] == 0
    print('on vs off', rel(on, off))
    assert torch.isfinite(on).all() and rel(on, off) <= 1e-3
