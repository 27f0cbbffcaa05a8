"""Fused eval-mode FeaturePropagation + classifier tail (csrc/fp_head_infer.hip, pcs_fp_head_infer) against
the tail written out in float64 on the CPU: inverse-distance weights from the float32 distances (+ 1e-9,
normalised), the gather of f2[b, idx], the concatenation [f1 | interp], 1x1 conv with bias, BN on the running
statistics and ReLU per hidden layer, the bias-only classifier.

Logits: norm-relative <= (nl + 1) * 2^-16 (2^-16 per split-bf16 matrix layer; a lost hi*lo term sits near
2e-3).  Models, tail fused against layered: <= 1e-3 (the model-level forward bar).
Measured on an MI355X (B, N, M, D1, ld1, nl, classes):
  (1, 100, 7, 0, -, 3, 13) 5.6e-06    (3, 257, 64, 32, 40, 4, 14) 6.0e-06
  (2, 128, 3, 4, 4, 1, 32) 5.1e-06    (2, 300, 16, 32, 32, 4, 1)  9.7e-06
Models at 2 x 1024: PointNetpp 1.1e-05, PointNetppMSG 1.9e-05, PointNeXt 1.1e-05."""
import pytest
import torch

import pcseg
from pcseg import engine
from pcseg.engine import fp_head_infer, fp_head_infer_ok, set_eval_fuse
from pcseg.synthetic import make_batch

DEV = 'cuda'
PROBE, INTERP = 'pcs::fp_head_infer_kernel', 'pcs::interp_cat_q_kernel'


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def tail_fp64(f1, f2, idx, dist, convs, bns):
    """f1 (B, N, D1) or None, f2 (B, M, 128), idx / dist (B, N, 3) -> (B * N, classes), [pre-activations]."""
    B, N, _ = idx.shape
    w = 1.0 / (dist.double() + 1e-9)
    w = w / w.sum(2, keepdim=True)
    nb = torch.stack([f2[b].double()[idx[b].long()] for b in range(B)])          # (B, N, 3, 128)
    x = (nb * w.unsqueeze(3)).sum(2)
    if f1 is not None:
        x = torch.cat([f1.double(), x], 2)
    x, zs = x.reshape(B * N, -1), []
    for i, conv in enumerate(convs):
        x = x @ conv.weight.detach().double().flatten(1).T + conv.bias.detach().double()
        if i < len(bns):
            bn = bns[i]
            zs.append((x - bn.running_mean.double()) / (bn.running_var.double() + bn.eps).sqrt()
                      * bn.weight.detach().double() + bn.bias.detach().double())
            x = torch.relu(zs[-1])
    return x, zs


@pytest.mark.gpu
@pytest.mark.parametrize('B,N,M,D1,ld1,nl,classes', [(1, 100, 7, 0, 0, 3, 13), (3, 257, 64, 32, 40, 4, 14),
                                                     (2, 128, 3, 4, 4, 1, 32), (2, 300, 16, 32, 32, 4, 1)])
def test_fp_head_infer_matches_fp64(B, N, M, D1, ld1, nl, classes):
    gen = torch.Generator().manual_seed(N + classes)
    convs, bns, cin = [], [], D1 + 128
    for _ in range(nl):
        conv, bn = torch.nn.Conv1d(cin, 128, 1), torch.nn.BatchNorm1d(128).eval()
        with torch.no_grad():
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) / cin ** 0.5)
            conv.bias.copy_(0.1 * torch.randn(128, generator=gen))
            bn.weight.copy_(torch.rand(128, generator=gen) + 0.5)
            bn.weight[1::7] *= -1                       # gamma < 0
            bn.weight[2::9] = 0                         # gamma == 0: the channel is relu(beta)
            bn.bias.copy_(torch.randn(128, generator=gen))
            bn.running_mean.copy_(0.5 * torch.randn(128, generator=gen))
            bn.running_var.copy_(torch.rand(128, generator=gen) + 0.3)
        convs.append(conv), bns.append(bn)
        cin = 128
    last = torch.nn.Conv1d(128, classes, 1)
    with torch.no_grad():
        last.weight.copy_(torch.randn(last.weight.shape, generator=gen) / 128 ** 0.5)
        last.bias.copy_(0.1 * torch.randn(classes, generator=gen))
    convs.append(last)
    # a gather from the wrong cloud is an O(1) error
    f2 = torch.randn(B, M, 128, generator=gen) + 3.0 * torch.arange(B).view(B, 1, 1)
    idx = torch.randint(0, M, (B, N, 3), generator=gen, dtype=torch.int32)
    idx[:, ::5, 1] = idx[:, ::5, 0]                     # a neighbour twice
    dist = torch.rand(B, N, 3, generator=gen) + 0.01
    dist[:, ::11, 0] = 0.0                              # a point on its neighbour
    f1 = torch.randn(B, N, D1, generator=gen) if D1 else None
    ref, zs = tail_fp64(f1, f2, idx, dist, convs, bns)
    rows = None
    if D1:
        rows = torch.full((B * N, ld1), 7.0)            # columns D1 .. ld1 are not channels
        rows[:, :D1] = f1.reshape(B * N, D1)
        rows = rows.to(DEV)
    convs, bns = [c.to(DEV) for c in convs], [b.to(DEV) for b in bns]
    assert fp_head_infer_ok(convs, bns, D1, 128)
    args = (rows, D1, f2.to(DEV), idx.to(DEV), dist.to(DEV), B, N, convs, bns)
    out = fp_head_infer(*args)
    with pcseg.replay(pcseg.Replay()) as rp:            # recording: the kernel's ReLU decisions, per hidden layer
        again = fp_head_infer(*args)
    print('rel vs fp64', rel(out, ref))
    assert out.shape == ref.shape and torch.isfinite(out).all()
    assert rel(out, ref) <= (nl + 1) * 2 ** -16
    assert torch.equal(out, again)
    assert len(rp.rec_act_mask) == nl
    for m, z in zip(rp.rec_act_mask, zs):
        assert m.shape == z.shape and torch.equal(m[z.abs() > 1e-2], z[z.abs() > 1e-2] > 0)


@pytest.mark.gpu
@pytest.mark.parametrize('cls', [pcseg.PointNetpp, pcseg.PointNetppMSG, pcseg.PointNeXt])
def test_family_tail_fused_only_in_eval_without_grad(cls):
    torch.manual_seed(5)
    model = cls(13).to(DEV)
    assert model.eval_fuse is False
    bns = [m for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
    starts = [torch.tensor([3, 11], dtype=torch.int32)] * 4
    g = torch.Generator().manual_seed(31)
    with torch.no_grad():
        for m in bns:
            m.momentum = 1.0
        with pcseg.replay(pcseg.Replay(fps_starts=starts)):
            model.train()(make_batch(2, 1024, seed=32)[0].to(DEV))      # calibrate the running statistics, then perturb
        for m in bns:
            m.running_mean.add_((torch.randn(m.running_mean.shape, generator=g) * 0.05).to(DEV))
            m.running_var.mul_((torch.rand(m.running_var.shape, generator=g) * 0.4 + 0.8).to(DEV))
    model.eval()
    pts = make_batch(2, 1024, seed=33)[0].to(DEV)

    def run(fuse, grad=False, train=False):
        set_eval_fuse(model, fuse)
        model.train(train)
        with torch.set_grad_enabled(grad), pcseg.replay(pcseg.Replay(fps_starts=starts)), engine.KernelProbe() as kp:
            y = model(pts)
        model.eval()
        names = [r[0] for r in kp.records()]
        return y.detach(), names.count(PROBE), names.count(INTERP)

    off, n_off, i_off = run(False)
    on, n_on, i_on = run(True)
    assert (n_off, n_on) == (0, 1) and i_on == i_off - 1
    assert run(True, grad=True)[1] == 0 and run(True, train=True)[1] == 0
    print('on vs off', rel(on, off))
    assert on.shape == off.shape and torch.isfinite(on).all() and rel(on, off) <= 1e-3
