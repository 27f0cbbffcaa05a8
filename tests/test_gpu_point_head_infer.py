"""Fused eval-mode PointNet segmentation head (csrc/point_head_infer.hip, pcs_point_head_infer) against
the head written out in float64 on the CPU: the concatenation [g expanded | p], 1x1 conv with bias, BN on
the running statistics, ReLU; the last layer bias only; then optionally exp / sum over the classes.

Logits: norm-relative <= 4 * 2^-16 ~ 6.1e-5 (2^-16 per split-bf16 matrix layer, four layers; a lost hi*lo
term sits near 2e-3).  Probabilities: <= 1e-3 (the model-level forward bar), rows sum to 1 within 1e-5.
Measured on an MI355X (B, N, ldp, classes, softmax):
  (1, 100, 64, 13, on) 5.1e-06    (3, 257, 72, 14, off) 7.1e-06
  (2, 128, 64, 32, on) 1.0e-05    (2, 300, 64, 1, off)  8.4e-06
PointNetSeg(14) at 2 x 300, head fused against layered: 3.2e-07 (feature_transform 2.9e-07)."""
import pytest
import torch

import pcseg
from pcseg import engine
from pcseg.engine import point_head_infer, point_head_infer_ok, set_eval_fuse

DEV = 'cuda'
PROBE = 'pcs::point_head_infer_kernel'
KG, KP = 1024, 64


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def head_fp64(g, p, convs, bns, softmax):
    """g (B, kg), p (B, N, kp) -> (B * N, classes)."""
    B, N, _ = p.shape
    x = torch.cat([g.double().view(B, 1, -1).expand(B, N, -1), p.double()], 2).reshape(B * N, -1)
    for i, conv in enumerate(convs):
        x = x @ conv.weight.detach().double().flatten(1).T + conv.bias.detach().double()
        if i < len(bns):
            bn = bns[i]
            x = torch.relu((x - bn.running_mean.double()) / (bn.running_var.double() + bn.eps).sqrt()
                           * bn.weight.detach().double() + bn.bias.detach().double())
    return torch.exp(x) / torch.exp(x).sum(1, keepdim=True) if softmax else x


@pytest.mark.gpu
@pytest.mark.parametrize('B,N,ldp,classes,softmax', [(1, 100, 64, 13, True), (3, 257, 72, 14, False),
                                                     (2, 128, 64, 32, True), (2, 300, 64, 1, False)])
def test_point_head_infer_matches_fp64(B, N, ldp, classes, softmax):
    gen = torch.Generator().manual_seed(N + classes)
    convs, bns, cin = [], [], KG + KP
    for n in (512, 256, 128):
        conv, bn = torch.nn.Conv1d(cin, n, 1), torch.nn.BatchNorm1d(n).eval()
        with torch.no_grad():
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) / cin ** 0.5)
            conv.bias.copy_(0.1 * torch.randn(n, generator=gen))
            bn.weight.copy_(torch.rand(n, generator=gen) + 0.5)
            bn.weight[1::7] *= -1                       # gamma < 0
            bn.weight[2::9] = 0                         # gamma == 0: the channel is relu(beta)
            bn.bias.copy_(torch.randn(n, generator=gen))
            bn.running_mean.copy_(0.5 * torch.randn(n, generator=gen))
            bn.running_var.copy_(torch.rand(n, generator=gen) + 0.3)
        convs.append(conv), bns.append(bn)
        cin = n
    last = torch.nn.Conv1d(cin, classes, 1)
    with torch.no_grad():
        last.weight.copy_(torch.randn(last.weight.shape, generator=gen) / cin ** 0.5)
        last.bias.copy_(0.1 * torch.randn(classes, generator=gen))
    convs.append(last)
    g = torch.randn(B, KG, generator=gen)               # per cloud: a bias from the wrong cloud is an O(1) error
    p = torch.randn(B, N, KP, generator=gen)
    ref = head_fp64(g, p, convs, bns, softmax)
    rows = torch.full((B * N, ldp), 7.0)                # columns kp .. ldp are not channels
    rows[:, :KP] = p.reshape(B * N, KP)
    convs, bns = [c.to(DEV) for c in convs], [b.to(DEV) for b in bns]
    assert point_head_infer_ok(convs, bns, KG, KP)
    out = point_head_infer(rows.to(DEV), KP, g.to(DEV), B, N, convs, bns, softmax=softmax)
    again = point_head_infer(rows.to(DEV), KP, g.to(DEV), B, N, convs, bns, softmax=softmax)
    print('rel vs fp64', rel(out, ref))
    assert out.shape == ref.shape and torch.isfinite(out).all()
    if softmax:
        assert rel(out, ref) <= 1e-3
        assert float((out.sum(1) - 1).abs().max()) <= 1e-5
    else:
        assert rel(out, ref) <= 4 * 2 ** -16
    assert torch.equal(out, again)


@pytest.mark.gpu
@pytest.mark.parametrize('feature_transform', [False, True])
def test_pointnet_head_fused_only_in_eval_without_grad(feature_transform):
    torch.manual_seed(3)
    model = pcseg.PointNetSeg(14, feature_transform=feature_transform).to(DEV).eval()
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
    assert (n_off, n_on) == (0, 1)
    assert run(True, grad=True)[1] == 0 and run(True, train=True)[1] == 0
    print('on vs off', rel(on, off))
    assert on.shape == off.shape and torch.isfinite(on).all() and rel(on, off) <= 1e-3
