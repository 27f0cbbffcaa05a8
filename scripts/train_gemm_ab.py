"""DGCNN training step with the head's wide GEMMs on the fp32 MFMA kernel (gemm_nt), on the split-bf16
kernel ('bf16x3') or with the head's weight gradients on their split-bf16 kernel as well ('bf16x3+wgrad')
(engine.set_train_gemm): one setting per process, alternate them from the shell.
DGCNNWithColor(k=20).train(), forward + masked cross-entropy + backward; 3 warm-up steps, then windows of
10 steps between device events (scripts/rows_infer_ab.py's protocol), and one probed step's wide-GEMM
launches in order (the launch probe's device events: name, microseconds, algorithmic GF): conv5, conv6,
conv7 forward, then conv7, conv6, conv5 data gradient; beside them the weight-gradient launches on plain
operands (conv7, conv6, conv5: wgrad_kernel<128, 128, 0, 0, 1> / wgrad_nt_kernel, or wgrad_bf16x3_kernel),
in-step times on the wgrad lane.  Last, outside the timing: one step of this setting and of the one it is
compared with ('fp32' <-> 'bf16x3', 'bf16x3+wgrad' -> 'bf16x3') on the same dropout seeds in the same
process, the norm-relative difference of the logits and of all parameter gradients.  Prints one JSON line."""
import argparse
import json
import os
import sys

sys.path[:0] = [os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'),
                os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '3d-semantic-segmentation-benchmark_amd')]
import torch  # noqa: E402
import pcseg  # noqa: E402
from pcseg import engine  # noqa: E402
from pcseg.synthetic import make_batch  # noqa: E402

WIDE = ('pcs::gemm_nt_kernel', 'pcs::gemm_nt_bf16x3_kernel')
WGRAD = ('pcs::wgrad_kernel<128, 128, 0, 0, 1>', 'pcs::wgrad_nt_kernel', 'pcs::wgrad_bf16x3_kernel')
OTHER = {'fp32': 'bf16x3', 'bf16x3': 'fp32', 'bf16x3+wgrad': 'bf16x3'}
ap = argparse.ArgumentParser()
ap.add_argument('--gemm', choices=engine.TRAIN_GEMM, default='fp32')
ap.add_argument('--batch', type=int, default=32)
ap.add_argument('--points', type=int, default=4096)
ap.add_argument('--k', type=int, default=20)
ap.add_argument('--windows', type=int, default=5)
ap.add_argument('--iters', type=int, default=10)
a = ap.parse_args()

torch.manual_seed(0)
model = pcseg.DGCNNWithColor(14, k=a.k).cuda().train()
engine.set_train_gemm(model, a.gemm)
pts, labels, lengths = make_batch(a.batch, a.points, seed=2000)
x = pts[:, :, :6].contiguous().transpose(1, 2).cuda()
lab, lengths = labels.float().cuda(), lengths.cuda()


def step():
    model.zero_grad()
    logits = model(x)[0]
    pcseg.masked_onehot_cross_entropy(logits, lab, lengths).backward()
    return logits


def seeded_step():
    torch.manual_seed(7)                       # the fused dropouts' mask seeds
    logits = step().detach().double()
    torch.cuda.synchronize()
    return logits, torch.cat([p.grad.double().flatten() for p in model.parameters()])


ms = []
for _ in range(3):
    step()
torch.cuda.synchronize()
for _ in range(a.windows):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        step()
    e1.record()
    e1.synchronize()
    ms.append(round(e0.elapsed_time(e1) / a.iters, 4))
with engine.KernelProbe() as kp:
    step()
    torch.cuda.synchronize()
launches, wgrads = ([(name.replace('pcs::', ''), round(sec * 1e6, 1), round(fl * 1e-9, 2))
                     for name, fl, _, sec in kp.records() if name.startswith(which)] for which in (WIDE, WGRAD))
mine = seeded_step()
engine.set_train_gemm(model, OTHER[a.gemm])
other = seeded_step()
rel = [float((m - o).norm() / o.norm()) for m, o in zip(mine, other)]
print(json.dumps({'gemm': a.gemm, 'batch': a.batch, 'points': a.points, 'k': a.k, 'ms_per_step': ms,
                  'logits_rel_vs_other': rel[0], 'grads_rel_vs_other': rel[1], 'wide_gemm_launches_us_GF': launches,
                  'plain_wgrad_launches_us_GF': wgrads}))
