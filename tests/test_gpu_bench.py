"""bench.py's plain run on the GPU, in a process of its own as it is used: `--steps` sets the
number of timed steps, the last stdout line carries the headline keys and `ms_per_step` and
none of `--full`'s extras, and `--dump-outputs DIR` leaves the last timed step's loss, logits,
flat gradients and flat parameters as finite float32 .npy files.  A small PointNet++ batch
(2 x 1024 points) keeps it to the process start plus a few steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


def test_plain_run_line_and_dumped_outputs(tmp_path):
    out = tmp_path / 'dump'
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    p = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1',
                        '--batch', '2', '--npoints', '1024', '--dump-outputs', str(out)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    rec = json.loads(p.stdout.rstrip('\n').splitlines()[-1])
    assert rec['steps'] == 3 and rec['warmup'] == 1 and rec['n_gpus'] == 1
    assert rec['unit'] == 'points/s' and rec['higher_is_better'] is True and rec['dtype'] == 'fp32'
    assert rec['ms_per_step'] > 0
    # value is the points of one step over the time of one step
    assert abs(rec['value'] - 2 * 1024 / (rec['ms_per_step'] * 1e-3)) <= 2e-3 * rec['value']
    assert rec['roofline'] is None and rec['cpu_baseline'] is None and rec['detail'] is None
    assert not {'secondary', 'other_configs', 'drop_in'} & set(rec)
    got = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert set(got) == {'loss', 'logits', 'grads', 'params'}
    for name, a in got.items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), name
    assert got['loss'].size == 1 and got['loss'] > 0
    assert got['logits'].size == 2 * 1024 * 14
    assert got['grads'].shape == got['params'].shape and got['grads'].ndim == 1
    assert np.abs(got['grads']).max() > 0 and np.abs(got['params']).max() > 0
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
