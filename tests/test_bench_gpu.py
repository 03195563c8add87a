"""bench.py end to end on the GPU, small: a plain run prints the headline line only and
--dump-outputs writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_with_dump_outputs(tmp_path):
    out = tmp_path / 'outputs'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3',
                        '--warmup', '1', '--batch', '32', '--dump-outputs', str(out)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, universal_newlines=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j['metric'] == 'CTC train-step frames/sec' and j['unit'] == 'frames/s'
    assert j['higher_is_better'] is True and j['dtype'] == 'bf16'
    assert j['steps'] == 3 and j['warmup'] == 1 and j['config']['optimizer_steps'] == 3
    assert j['ms_per_step'] > 0
    assert abs(j['value'] - 32 * 1000 / (j['ms_per_step'] * 1e-3)) <= 1e-6 * j['value']
    for k in ('roofline', 'roofline_bichar', 'decode'):         # --full only
        assert k not in j
    assert j['extra_workloads'] == [] and j['cpu_baseline'] is None

    files = sorted(os.listdir(str(out)))
    assert 'out.loss.npy' in files and 'state.decoder.fc.0.module.0.weight.npy' in files
    assert 'grad.encoder.rnns.0.rnn.weight_hh_l0.npy' in files
    assert sum(os.path.getsize(str(out / f)) for f in files) <= 64 * 10 ** 6
    for f in files:
        a = np.load(str(out / f))
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
    assert float(np.load(str(out / 'out.loss.npy'))) == pytest.approx(j['config']['final_loss'], rel=1e-6)
    g = np.load(str(out / 'grad.decoder.fc.0.module.0.weight.npy'))
    assert g.shape == (49, 320) and np.abs(g).max() > 0
