"""bench.py --dump-outputs: what the last timed step computed, written as float .npy files so that two builds can be compared
output for output (bench.dump_outputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_names_dtypes_and_fixed_samples(tmp_path):
    import bench
    g = torch.Generator().manual_seed(0)
    params = [torch.nn.Parameter(torch.randn((1500, 1000), generator=g)), torch.nn.Parameter(torch.randn((7,), generator=g))]
    params[0].grad = torch.randn((1500, 1000), generator=g)   # params[1] has no gradient: written as zeros
    last = {'loss': torch.tensor(3.5, requires_grad=True) * 2,
            'losses': {'loss_ce': torch.tensor(1.0), 'loss_giou': torch.tensor(2.0, dtype=torch.float64)},
            'out': {'pred_logits': torch.randn((8, 100, 2), generator=g).bfloat16(),
                    'aux_outputs': [{'pred_boxes': torch.randn((8, 100, 2), generator=g)}],
                    '_svol_stacked': (torch.randn((3,), generator=g),),
                    'big': torch.randn((3_000_000,), generator=g)}}
    shapes = bench.dump_outputs(str(tmp_path / 'a'), last, params)
    assert shapes == {'loss': [], 'losses.loss_ce': [], 'losses.loss_giou': [], 'out.aux_outputs.0.pred_boxes': [8, 100, 2],
                      'out.big.sample': [bench.DUMP_SAMPLE], 'out.pred_logits': [8, 100, 2],
                      'grad_sample': [bench.DUMP_SAMPLE]}
    files = sorted(os.listdir(tmp_path / 'a'))
    assert files == sorted(n + '.npy' for n in shapes)
    arrays = {f[:-4]: np.load(tmp_path / 'a' / f) for f in files}
    assert arrays['losses.loss_giou'].dtype == np.float64
    assert all(x.dtype == np.float32 for k, x in arrays.items() if k != 'losses.loss_giou')
    assert arrays['loss'].item() == 7.0
    np.testing.assert_array_equal(arrays['out.pred_logits'], last['out']['pred_logits'].float().numpy())
    # the sample: entries of the flattened vector (parameters in the optimiser's order) at positions drawn once from a fixed seed
    flat = torch.cat([params[0].grad.reshape(-1), torch.zeros(7)]).numpy()
    idx = np.sort(np.random.default_rng(0).choice(flat.size, size=bench.DUMP_SAMPLE, replace=False))
    np.testing.assert_array_equal(arrays['grad_sample'], flat[idx])
    # ... the same in a second dump
    bench.dump_outputs(str(tmp_path / 'b'), last, params)
    for f in files:
        np.testing.assert_array_equal(arrays[f[:-4]], np.load(tmp_path / 'b' / f))


@pytest.mark.gpu
@pytest.mark.parametrize('deterministic', [False, True], ids=['default', 'deterministic'])
def test_bench_dump_is_the_same_from_run_to_run(tmp_path, deterministic):
    """Two bench runs with the same arguments dump the same arrays: every step of a dumping run starts from the seeded initial
    parameters, so the forward (no atomics) and the losses are bit-identical and the gradients equal to rounding — the backward's
    fp32 atomics; under SVOL_DETERMINISTIC=1 (every reduction in a fixed order) everything is bit-identical.  --steps is the
    number of timed steps and the dump stays within 64 MB."""
    env = dict(os.environ)
    env.pop('SVOL_DETERMINISTIC', None)
    if deterministic:
        env['SVOL_DETERMINISTIC'] = '1'
    runs = []
    for i in range(2):
        d = tmp_path / ('run%d' % i)
        p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '4', '--warmup', '2', '--no-cpu-baseline',
                            '--dump-outputs', str(d)], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        line = json.loads(p.stdout.strip().splitlines()[-1])
        assert line['steps'] == 4 and len(line['ms_per_step_blocks']) == 1 and line['ms_per_step'] > 0
        arrays = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
        assert set(arrays) == set(line['dumped_outputs']['arrays'])
        assert {'loss', 'out.pred_logits', 'out.pred_boxes', 'grad_sample'} <= set(arrays)
        assert any(k.startswith('losses.') for k in arrays) and any(k.startswith('out.aux_outputs.') for k in arrays)
        assert all(x.dtype in (np.float32, np.float64) and np.isfinite(x).all() for x in arrays.values())
        assert sum(x.nbytes for x in arrays.values()) <= 64 << 20
        assert np.abs(arrays['grad_sample']).max() > 0
        runs.append(arrays)
    for k in runs[0]:
        a, b = runs[0][k], runs[1][k]
        if k == 'grad_sample' and not deterministic:
            scale = float(np.abs(a).max())
            assert float(np.abs(a.astype(np.float64) - b).max()) <= 1e-5 * scale, (k, float(np.abs(a.astype(np.float64) - b).max()), scale)
        else:
            np.testing.assert_array_equal(a, b, err_msg=k)
