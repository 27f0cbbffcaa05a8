"""bench.py's final stdout line stays a compact JSON object the driver can parse (round 5's
32 KB line overflowed the driver's ~10 KB stdout tail): built from a canned full record (the
round-5 default run's, profiles/r05_bench_default.json), it is under 4096 bytes, is the last
stdout line, carries the contract's keys plus the compact roofline and CPU baseline of both
halves of the metric, and names the detail file that holds the rest."""
import json
import os
import sys

from conftest import REPO

sys.path.insert(0, REPO)
import bench  # noqa: E402

CANNED = os.path.join(REPO, 'profiles', 'r05_bench_default.json')


def _canned():
    full = json.load(open(CANNED))
    for r in [full, full['secondary']] + list(full['other_configs'].values()):
        r['config'].setdefault('rccl_world', 1)
        roof = r['roofline']
        roof['committed_profile_avg_us'] = roof.pop('rocprof_avg_launch_us', None)
    return full


def test_line_is_compact_last_and_complete(tmp_path, capsys):
    full = _canned()
    det = tmp_path / 'bench_detail.json'
    line = bench.emit_line(full, str(det))
    out = capsys.readouterr().out
    assert out.rstrip('\n').splitlines()[-1] == line
    assert len(line.encode()) <= 4096, len(line)
    rec = json.loads(line)
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better',
              'scaling', 'vs_baseline', 'dtype', 'data', 'config'):
        assert k in rec, k
    assert rec['metric'] == bench.METRIC and rec['value'] == full['value']
    assert 'workload' in rec['config']
    for blk in (rec, rec['secondary']):
        roof = blk['roofline']
        for k in ('kernel', 'bound', 'achieved', 'peak', 'unit', 'frac', 'traffic', 'avg_launch_us'):
            assert k in roof, k
        assert abs(roof['frac'] - roof['achieved'] / roof['peak']) < 1e-3
        assert blk['cpu_baseline']['value'] > 0 and blk['cpu_baseline']['cores'] > 0
    assert rec['secondary']['ms_per_step'] == full['secondary']['ms_per_step']
    assert set(rec['other_configs']) == {'pointnetpp_msg', 'pointnext'}
    for v in rec['other_configs'].values():
        assert set(v) == {'value', 'ms_per_step', 'frac', 'drop_in_ms'}
    # the detail file holds the full record
    assert json.load(open(det))['roofline']['top_kernels'] == full['roofline']['top_kernels']
    assert rec['detail'] == os.path.relpath(str(det), REPO)


def test_plain_record_has_the_contract_keys_and_no_extras():
    """The line of a run without --full: one workload, no roofline, CPU baseline, drop-in,
    secondary, other configs or detail file -- and still the contract's keys."""
    w = {'value': 1.0e7, 'unit': 'points/s', 'ms_per_step': 13.1, 'config': {'workload': 'w', 'model': 'PointNetpp'},
         'host_enqueue_ms_per_step': 3.0, 'host_runahead_wait_ms_per_step': 0.0, 'roofline': None,
         'step_roofline': None}
    args = type('A', (), {'model': 'pointnetpp', 'steps': 7, 'warmup': 2})()
    full = bench.full_record({'pointnetpp': w}, {}, args, 1, 1, ['pointnetpp'], [])
    rec = bench.compact_line(full, None)
    for k, v in (('metric', bench.METRIC), ('value', 1.0e7), ('unit', 'points/s'), ('higher_is_better', True),
                 ('dtype', 'fp32'), ('ms_per_step', 13.1), ('steps', 7), ('warmup', 2), ('n_gpus', 1)):
        assert rec[k] == v, k
    assert rec['roofline'] is None and rec['cpu_baseline'] is None and rec['detail'] is None
    assert not {'secondary', 'other_configs', 'drop_in'} & set(rec)


def test_extra_workloads_need_full():
    import pytest
    for flag, v in (('--secondary', 'dgcnn'), ('--others', 'pointnext')):
        with pytest.raises(SystemExit, match='needs --full'):
            bench.main(['--gpus', '1', flag, v])


def test_dump_outputs_writes_float_npy_within_the_limit(tmp_path):
    import numpy as np
    import torch
    arrays = {'loss': torch.tensor(0.5), 'big': torch.arange(1000, dtype=torch.float32).reshape(10, 100),
              'ints': torch.arange(6, dtype=torch.int32), 'wide': torch.arange(4, dtype=torch.float64)}
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), arrays, limit=4 * 400)     # 400 bytes each: 100 fp32 of `big`
    got = {n: np.load(tmp_path / 'a' / f'{n}.npy') for n in arrays}
    assert got['loss'].dtype == np.float32 and got['loss'].shape == () and got['loss'] == 0.5
    assert got['ints'].dtype == np.float32 and got['ints'].tolist() == [0, 1, 2, 3, 4, 5]
    assert got['wide'].dtype == np.float64 and got['wide'].tolist() == [0, 1, 2, 3]
    big = got['big']
    assert big.dtype == np.float32 and big.shape == (100,)
    assert np.all(np.diff(big) > 0) and set(big.tolist()) <= set(range(1000))    # a sample of the elements, in order
    assert np.array_equal(big, np.load(tmp_path / 'b' / 'big.npy'))              # the same sample every time
    assert sum(a.nbytes for a in got.values()) <= 4 * 400


def test_line_trims_when_strings_grow():
    full = _canned()
    full['cpu_baseline']['sample'] = 'x' * 5000
    full['secondary']['config']['workload'] = 'y' * 1500
    line = json.dumps(bench.compact_line(full, None), separators=(',', ':'))
    assert len(line.encode()) <= 4096
    json.loads(line)
