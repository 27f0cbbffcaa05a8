"""Split-bf16 eval-mode conv + BN + activation on rows (csrc/rows_infer.hip, pcs_rows_infer) against the
formula Y = act(s o (X W^T + bias - running_mean) + beta), s = gamma / sqrt(running_var + eps), written
out in float64 on the CPU, and against the layered fp32 engine path.  Norm-relative bound: the 1e-4 of
the other eval kernels' tests; the three-term split sits near 4.5e-6 and a dropped cross term near 2e-3.

M = 301 rows is no multiple of the 128-row tile (or of a wave's 64 / 32); cin 20 is less than one K slab
of 32, 200 no multiple of 16 or 32, 1408 DGCNN's conv6; cout 12 is less than one MFMA tile, 132 crosses a
128-column block tile."""
import pytest
import torch

import pcseg
from pcseg import _lib, engine
from pcseg.engine import (KernelProbe, linear_rows, rows_infer, rows_infer_ok, rows_infer_stack, set_eval_gemm,
                          shared_mlp, storage_alias)
from pcseg.synthetic import make_batch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TOL = 1e-4
M = 301
NEG, ZERO = [1, 6], [2, 9]                   # gamma < 0 / gamma == 0 columns
ACTS = {'relu': lambda y: y.relu(), 'lrelu': lambda y: torch.where(y > 0, y, 0.2 * y), 'none': lambda y: y}


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _init(cin, cout, with_bn, seed):
    """Post-ReLU-like rows, a seeded conv with bias, an eval-mode BN with a non-trivial state (or None) and
    the fp64 pre-activation (M, cout)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, cin, generator=g).relu()
    conv, bn = torch.nn.Conv1d(cin, cout, 1), None
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / cin ** 0.5)
        conv.bias.copy_(0.1 * torch.randn(cout, generator=g))
        y = x.double() @ conv.weight.double().flatten(1).T + conv.bias.double()
        if with_bn:
            bn = torch.nn.BatchNorm1d(cout).eval()
            bn.weight.copy_(torch.rand(cout, generator=g) + 0.5)
            bn.weight[NEG] *= -1
            bn.weight[ZERO] = 0
            bn.bias.copy_(torch.randn(cout, generator=g))
            bn.running_mean.copy_(0.5 * torch.randn(cout, generator=g))
            bn.running_var.copy_(torch.rand(cout, generator=g) + 0.3)
            y = (y - bn.running_mean.double()) / (bn.running_var.double() + bn.eps).sqrt() * bn.weight.double() \
                + bn.bias.double()
    return x, conv, bn, y


@pytest.mark.parametrize('cin,cout,act,with_bn,blocks', [
    (20, 12, 'relu', True, False), (200, 132, 'lrelu', True, False), (1408, 512, 'none', True, False),
    (1408, 132, 'relu', True, False), (200, 12, 'none', False, False), (20, 512, 'lrelu', True, True),
    (200, 132, 'relu', True, True)])
def test_rows_infer_matches_fp64_and_layered_path(cin, cout, act, with_bn, blocks):
    x, conv, bn, y = _init(cin, cout, with_bn, seed=cin + cout)
    ref = ACTS[act](y)
    conv = conv.to(DEV)
    bn = bn.to(DEV) if bn is not None else None
    xd, out = x.to(DEV), None
    if blocks:      # X and Y as column blocks of wider buffers
        xbuf = torch.full((M, cin + 12), float('nan'), device=DEV)
        ybuf = torch.full((M, cout + 8), float('nan'), device=DEV)
        xd, out = storage_alias(xbuf, 8, cin), storage_alias(ybuf, 4, cout)
        xd.copy_(x)
    assert rows_infer_ok(conv, bn, cin)
    got = rows_infer(xd, cin, conv, bn, act, 0.2, out=out)
    with torch.no_grad():
        layered = shared_mlp(xd, cin, [conv], [bn], act, 0.2) if with_bn else linear_rows(xd, conv)
    print('rel vs fp64', rel(got, ref), 'vs layered', rel(got, layered))
    assert got.shape == ref.shape and torch.isfinite(got).all()
    assert rel(got, ref) < TOL and rel(got, layered) < TOL
    if with_bn:
        beta = ACTS[act](bn.bias.detach()[ZERO])
        assert torch.equal(got[:, ZERO], beta.expand(M, -1))
    if blocks:
        assert torch.isnan(ybuf[:, :4]).all() and torch.isnan(ybuf[:, 4 + cout:]).all()
        assert torch.equal(ybuf[:, 4:4 + cout], got)


def test_rows_infer_stack_chains_layers():
    x, c1, b1, _ = _init(200, 132, True, seed=3)
    _, c2, b2, _ = _init(132, 12, True, seed=4)
    convs, bns = [c1.to(DEV), c2.to(DEV)], [b1.to(DEV), b2.to(DEV)]
    got = rows_infer_stack(x.to(DEV), 200, convs, bns, 'relu')
    with torch.no_grad():
        layered = shared_mlp(x.to(DEV), 200, convs, bns, 'relu')
    print('stack rel vs layered', rel(got, layered))
    assert got.shape == (M, 12) and rel(got, layered) < TOL


@pytest.mark.parametrize('name', ['dgcnn', 'pointnetpp'])
def test_models_dispatch_eval_no_grad_to_rows_infer(name):
    g = torch.Generator().manual_seed(41)
    if name == 'dgcnn':
        model, x, covered = pcseg.DGCNNWithColor(13, k=20).to(DEV), torch.randn(2, 6, 128, generator=g).to(DEV), 3
    else:
        model, x, covered = pcseg.PointNetpp(13).to(DEV), make_batch(2, 1024, seed=33)[0].to(DEV), 10
    bns = [m for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
    starts = [torch.tensor([3, 11], dtype=torch.int32)] * 4
    with torch.no_grad():
        for m in bns:
            m.momentum = 1.0
        with pcseg.replay(pcseg.Replay(fps_starts=starts)):
            model.train()(x)                 # calibrate the running statistics, then perturb
        for m in bns:
            m.running_mean.add_((torch.randn(m.running_mean.shape, generator=g) * 0.05).to(DEV))
            m.running_var.mul_((torch.rand(m.running_var.shape, generator=g) * 0.4 + 0.8).to(DEV))
    model.eval()
    outs, names, grads = {}, {}, {}
    for mode in ('never', 'bf16x3', 'fp32'):
        if mode != 'never':
            set_eval_gemm(model, mode, min_rows=0)       # these models' row counts are below the default crossover
        with torch.no_grad(), pcseg.replay(pcseg.Replay(fps_starts=starts)), KernelProbe() as kp:
            o = model(x)
        outs[mode] = o[0] if isinstance(o, tuple) else o
        names[mode] = [r[0] for r in kp.records()]
        with pcseg.replay(pcseg.Replay(fps_starts=starts)):
            o = model(x)
        grads[mode] = (o[0] if isinstance(o, tuple) else o).detach()
    gemms = {k: sum(n.startswith(('pcs::gemm_rows_kernel', 'pcs::fwd_dma_kernel', 'pcs::gemm_nt_kernel')) for n in v)
             for k, v in names.items()}
    new = {k: sum(n.startswith('pcs::rows_infer_kernel') for n in v) for k, v in names.items()}
    print('logits rel', rel(outs['bf16x3'], outs['never']), 'engine GEMMs', gemms, 'rows_infer launches', new)
    assert new == {'never': 0, 'bf16x3': covered, 'fp32': 0}
    assert gemms['bf16x3'] == gemms['never'] - covered and gemms['fp32'] == gemms['never']
    assert torch.isfinite(outs['bf16x3']).all() and rel(outs['bf16x3'], outs['never']) < TOL
    assert not torch.equal(outs['bf16x3'], outs['never']) and torch.equal(outs['fp32'], outs['never'])
    assert torch.equal(grads['bf16x3'], grads['never'])          # a backward is possible: the flag changes nothing


def test_rows_infer_argument_checks():
    lib = _lib.load()
    fake = 0x1000                       # never dereferenced: every call fails its checks first

    def rec(cin, cout, use_batch=0):
        return engine._REC.pack(fake, cin, cin, cout, 0, fake, fake, fake, fake, 0, 0.0, 1e-5, use_batch, 0, 0.0,
                                0, 0, 0, 0, 0, 0, 0.0, 0, 0, 0)
    for xp, r in ((fake, rec(64, 32, use_batch=1)), (fake, rec(6, 32)), (fake, rec(64, 30)), (None, rec(64, 32))):
        assert lib.pcs_rows_infer(xp, 64, 128, r, fake, 32, None) != 0
        assert b'pcs_rows_infer' in lib.pcs_last_error()
    x, conv, bn, _ = _init(20, 12, True, seed=1)
    odd = torch.nn.Conv1d(6, 12, 1)
    assert rows_infer_ok(conv, bn, 20) and rows_infer_ok(conv, None, 20)
    assert not rows_infer_ok(conv, bn, 20, rows=4096) and rows_infer_ok(conv, bn, 20, rows=16384)
    assert not rows_infer_ok(conv, bn.train(), 20) and not rows_infer_ok(odd, None, 6)
    with pytest.raises(ValueError):
        rows_infer(x.to(DEV), 20, conv.to(DEV), bn.to(DEV), 'relu')       # training-mode BN
    with pytest.raises(ValueError):
        rows_infer(x[:, :6].to(DEV), 6, odd.to(DEV), None, 'none')
