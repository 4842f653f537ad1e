"""bench.py as every change is measured with it: a plain run times ONE region of exactly --steps iterations, reports ms_per_step and
nothing beyond the headline; --dump-outputs writes what the last timed iteration computed (float32 .npy files, at most 64 MB), and two
runs with the same arguments write the same arrays."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_exactly_steps_and_dumps_the_last_step(tmp_path):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')

    def run(dump):
        r = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', '3', '--warmup', '1', '--dump-outputs', str(dump)],
                           cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith('{')]
        assert len(lines) == 1, r.stdout.decode()[-2000:]
        arrays = {f[:-len('.npy')]: np.load(os.path.join(str(dump), f)) for f in os.listdir(str(dump)) if f.endswith('.npy')}
        return json.loads(lines[0]), arrays
    out, arrays = run(tmp_path / 'first')
    assert out['unit'] == 'images/sec' and out['higher_is_better'] is True and out['dtype'] == 'f32' and 'metric' in out
    assert out['steps'] == 3 and out['warmup'] == 1
    assert out['timing']['regions'] == 1 and out['timing']['steps_per_region'] == 3
    assert out['ms_per_step'] > 0 and abs(out['value'] - 64 * 1e3 / out['ms_per_step']) <= 1e-6 * out['value']
    for k in ('roofline', 'config3_bf16', 'b8_per_gpu', 'next_rows', 'cpu_baseline', 'cpu_baseline_b64', 'dp_preflight'):
        assert k not in out, k
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert all(np.isfinite(a).all() for a in arrays.values()), [k for k, a in arrays.items() if not np.isfinite(a).all()]
    assert arrays['d_G'].shape == (64, 64, 64, 3) and arrays['g_G'].shape == (64, 64, 64, 3)
    for k in ('d_D_loss', 'd_wdist', 'g_G_loss', 'g_G_kl_loss', 'kt'):
        assert arrays[k].size == 1, k
    assert arrays['d_weights_sample'].shape == (1 << 20,) and arrays['g_weights_sample'].shape == (1 << 20,)
    assert np.abs(arrays['d_G']).max() <= 1.0         # tanh output
    # the inputs are seeded (batch, weights, and the conditioning noise the iteration draws itself): a second run computes the same bits
    _, again = run(tmp_path / 'second')
    assert sorted(again) == sorted(arrays)
    assert [k for k in sorted(arrays) if not np.array_equal(arrays[k], again[k])] == []
