"""Fused eval-mode grouped MLP + max-pool (csrc/group_mlp_infer.hip, pcs_group_mlp_infer) against the
reference SetAbstraction stack (models/utils/common.py:37-71, 125-150, 180-214 under eval()) written
out in float64 on the CPU with the same index table: gather [(xyz - cent) (/ r), feats], 1x1 conv with
bias, BN on the running statistics, ReLU, max over K.  Norm-relative bound: the 1e-4 of
test_gpu_edgeconv_infer.py (the same fp32-MFMA arithmetic).

B = 2 clouds of N = 97 points and C = 37 centroids: 74 groups are no multiple of the 4 (K = 32) or 8
(K = 16) groups of a 128-row tile, so the last tile is ragged, and the clouds are aligned to nothing."""
import pytest
import torch

import pcseg
from pcseg import _lib, engine, ops
from pcseg.engine import group_mlp_infer, group_mlp_infer_ok, set_eval_fuse
from pcseg.synthetic import make_batch

DEV = 'cuda'
TOL = 1e-4
B, N, C, R = 2, 97, 37, 0.4
NEG, ZERO = [1, 6], [2, 9]                   # gamma < 0 (every layer) / gamma == 0 (last layer)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _init(mini, g):
    """Seeded weights, conv biases and a non-trivial BN state for a MiniPointNet."""
    with torch.no_grad():
        for li, (conv, bn) in enumerate(zip(mini.conv, mini.batch)):
            n = conv.weight.shape[0]
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / conv.weight.shape[1] ** 0.5)
            conv.bias.copy_(0.1 * torch.randn(n, generator=g))
            bn.weight.copy_(torch.rand(n, generator=g) + 0.5)
            bn.weight[NEG] *= -1
            if li == len(mini.conv) - 1:
                bn.weight[ZERO] = 0
            bn.bias.copy_(torch.randn(n, generator=g))
            bn.running_mean.copy_(0.5 * torch.randn(n, generator=g))
            bn.running_var.copy_(torch.rand(n, generator=g) + 0.3)
    return mini.eval()


def _case(D, widths, K, normalize, seed):
    """xyz, feats, cent, idx (B, C, K) int32, an eval-mode MiniPointNet and the fp64 reference (B*C, cout)."""
    g = torch.Generator().manual_seed(seed)
    xyz, feats, cent = torch.rand(B, N, 3, generator=g), torch.randn(B, N, D, generator=g), torch.rand(B, C, 3, generator=g)
    idx = torch.randint(0, N, (B, C, K), generator=g, dtype=torch.int32)
    m = _init(pcseg.MiniPointNet(3 + D, widths), g)
    bi = torch.arange(B)[:, None, None]
    rel_xyz = xyz.double()[bi, idx.long()] - cent.double()[:, :, None]
    x = torch.cat([rel_xyz / R if normalize else rel_xyz, feats.double()[bi, idx.long()]], -1)      # (B, C, K, 3 + D)
    for conv, bn in zip(m.conv, m.batch):
        z = x @ conv.weight.detach().double().flatten(1).T + conv.bias.detach().double()
        x = torch.relu((z - bn.running_mean.double()) / (bn.running_var.double() + bn.eps).sqrt()
                       * bn.weight.detach().double() + bn.bias.detach().double())
    return xyz, feats, cent, idx, m, x.max(2).values.reshape(B * C, -1)


@pytest.mark.gpu
@pytest.mark.parametrize('D,widths,K,normalize', [(6, [32, 32, 64], 32, False), (64, [64, 64, 128], 32, True),
                                                  (6, [16, 16, 32], 16, False), (64, [64], 16, True),
                                                  (128, [128], 32, True)])
def test_group_mlp_infer_matches_fp64_and_layered_path(D, widths, K, normalize):
    xyz, feats, cent, idx, m, ref = _case(D, widths, K, normalize, seed=D + K + len(widths))
    m = m.to(DEV)
    t = [v.to(DEV) for v in (xyz, feats, cent, idx)]
    assert group_mlp_infer_ok(m.conv, m.batch, 3 + D, K)
    out = group_mlp_infer(*t, R, normalize, m.conv, m.batch)
    with torch.no_grad():
        layered = m.forward_rows(ops.group_rows(*t, R, normalize), 3 + D, pool_k=K)
    print('rel vs fp64', rel(out, ref), 'vs layered', rel(out, layered))
    assert out.shape == ref.shape and torch.isfinite(out).all()
    assert rel(out, ref) < TOL and rel(out, layered) < TOL
    beta = m.batch[-1].bias.detach()[ZERO]
    assert torch.equal(out[:, ZERO], torch.relu(beta).expand(B * C, -1))


@pytest.mark.gpu
def test_group_mlp_infer_weight_and_feats_at_storage_end():
    D, K = 64, 32
    xyz, feats, cent, idx, m, ref = _case(D, [64, 64, 128], K, True, seed=9)
    m = m.to(DEV)
    conv = m.conv[-1]
    store = torch.full((256 + conv.weight.numel(),), float('nan'), device=DEV)   # the weight ends where its storage ends
    store[256:].copy_(conv.weight.detach().flatten())
    conv.weight = torch.nn.Parameter(store[256:].view_as(conv.weight))
    fbuf = torch.full((256 + feats.numel(),), float('nan'), device=DEV)          # feats: the buffer's last bytes
    fin = fbuf[256:].view(B, N, D)
    fin.copy_(feats)
    out = group_mlp_infer(xyz.to(DEV), fin, cent.to(DEV), idx.to(DEV), R, True, m.conv, m.batch)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and rel(out, ref) < TOL
    assert torch.isnan(store[:256]).all() and torch.isnan(fbuf[:256]).all()


@pytest.mark.gpu
def test_set_abstraction_dispatches_eval_no_grad_to_fused_kernel():
    xyz, feats, cent, idx, _, _ = _case(6, [32, 32, 64], 32, False, seed=4)
    sa = pcseg.SetAbstraction(C, R, 9, [32, 32, 64])
    _init(sa.point_net, torch.Generator().manual_seed(5))
    sa = sa.to(DEV).eval()
    pn = sa.point_net
    xyz, feats, cent, idx = (v.to(DEV) for v in (xyz, feats, cent, idx))
    state = [v.clone() for bn in pn.batch for v in (bn.running_mean, bn.running_var, bn.num_batches_tracked)]
    with torch.no_grad():
        off = sa(xyz, feats, geo=(cent, idx))[1]
        assert torch.equal(off.reshape(B * C, -1), pn.forward_rows(ops.group_rows(xyz, feats, cent, idx, R, False), 9, pool_k=32))
        set_eval_fuse(sa)
        on = sa(xyz, feats, geo=(cent, idx))[1]
    assert pn.eval_fuse and not on.requires_grad
    assert torch.equal(on.reshape(B * C, -1), group_mlp_infer(xyz, feats, cent, idx, R, False, pn.conv, pn.batch))
    assert rel(on, off) < TOL
    og = sa(xyz, feats.clone().requires_grad_(True), geo=(cent, idx))[1]      # a backward is possible: layered path
    assert og.requires_grad and rel(og.detach(), off) < TOL
    for a, b in zip(state, [v for bn in pn.batch for v in (bn.running_mean, bn.running_var, bn.num_batches_tracked)]):
        assert torch.equal(a, b)
    assert group_mlp_infer_ok(pn.conv, pn.batch, 9, 32) and not group_mlp_infer_ok(pn.conv, pn.batch, 9, 20)
    wide = pcseg.MiniPointNet(9, [32, 256]).eval()
    assert not group_mlp_infer_ok(wide.conv, wide.batch, 9, 32)
    assert not group_mlp_infer_ok(pn.conv, sa.train().point_net.batch, 9, 32)


@pytest.mark.gpu
def test_pointnetpp_logits_with_eval_fuse_match_layered_eval():
    model = pcseg.PointNetpp(13).to(DEV)
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
    logits = []
    for on in (False, True):
        set_eval_fuse(model, on)
        with torch.no_grad(), pcseg.replay(pcseg.Replay(fps_starts=starts)):
            logits.append(model(pts))
    print('logits rel', rel(logits[1], logits[0]))
    assert torch.isfinite(logits[1]).all() and rel(logits[1], logits[0]) < 1e-3
    assert not torch.equal(logits[1], logits[0])          # the fused kernel did run


def test_group_mlp_infer_argument_checks_without_gpu():
    lib = _lib.load()
    fake = 0x1000                       # never dereferenced: every call fails its checks first

    def rec(cin, cout, use_batch=0):
        return engine._REC.pack(fake, cin, cin, cout, 0, fake, fake, fake, fake, 0, 0.0, 1e-5, use_batch, 0, 0.0,
                                0, 0, 0, 0, 0, 0, 0.0, 0, 0, 0)
    too_big = [rec(131, 128), rec(128, 128), rec(128, 128)]          # 207 KB of folded weights alone
    for K, D, recs, ix in ((20, 6, [rec(9, 32)], fake), (32, 6, [rec(9, 6)], fake), (32, 6, [rec(9, 32)], None),
                           (32, 6, [rec(9, 32, use_batch=1)], fake), (32, 128, too_big, fake)):
        rc = lib.pcs_group_mlp_infer(fake, fake, fake, ix, 1, 64, 8, K, D, 0.4, 0, b''.join(recs), len(recs), fake, None)
        assert rc != 0
        assert b'pcs_group_mlp_infer' in lib.pcs_last_error()
