"""GPU (-m gpu): the plain ``bench.py`` run -- one JSON line with the headline fields, --steps timed steps, and
--dump-outputs writing the generator output of the last timed step, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1'] + list(args), cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert p.returncode == 0 and len(lines) == 1, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
    return json.loads(lines[0])


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    d = _bench('--steps', '3', '--warmup', '1', '--dump-outputs', str(tmp_path / 'a'))
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in d, k
    assert d['unit'] == 'frames/s' and d['higher_is_better'] is True
    assert d['steps'] == 3 and d['warmup'] == 1 and d['value'] > 0 and d['ms_per_step'] > 0
    assert abs(d['value'] * d['ms_per_step'] / 1e3 - 16) < 0.05, d          # 16 frames per timed step
    # a plain run carries none of the --full legs
    assert d['roofline'] is None and d['parity_linf_vs_oracle'] is None, d
    assert not any(k in d for k in ('exact_fp32', 'train_step', 'train_step_bf16', 'stream', 'cpu_baseline')), sorted(d)
    y = np.load(tmp_path / 'a' / 'generator_output.npy')
    assert y.dtype == np.float32 and y.shape == (16, 1, 256, 256) and np.isfinite(y).all()
    assert 0.0 < float(np.abs(y).max()) <= 1.0                                # tanh output
    # the same arguments but other step counts: same weights and inputs, so the same output
    _bench('--steps', '1', '--warmup', '0', '--dump-outputs', str(tmp_path / 'b'))
    y2 = np.load(tmp_path / 'b' / 'generator_output.npy')
    assert float(np.abs(y2 - y).max()) < 1e-4
