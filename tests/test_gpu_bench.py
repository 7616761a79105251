"""GPU: a plain `bench.py` run at a tiny batch -- the result line's fields, the work it leaves to
--full, and --dump-outputs (the timed path's outputs of the last step, consistent with the packed
rows and with a pipeline run in this process on the same seeded inputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from mec import engine, synthetic as syn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 8


@pytest.fixture(scope='module')
def plain_run(tmp_path_factory):
    d = tmp_path_factory.mktemp('bench') / 'dump'
    env = dict(os.environ)
    env.pop('WORLD_SIZE', None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1',
                        '--batch', str(B), '--dump-outputs', str(d)], capture_output=True, text=True, timeout=110,
                       env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0]), d


def test_plain_line_fields_and_what_full_keeps(plain_run):
    r, _ = plain_run
    assert r['steps'] == 3 and r['warmup'] == 1 and r['n_gpus'] == 1 and r['per_rank_batch'] == B
    assert r['precision'] == 'fp32x3' and r['dtype'].startswith('fp32') and r['unit'] == 'samples/s'
    assert r['higher_is_better'] is True and r['ms_per_step'] > 0
    assert r['value'] == pytest.approx(B * 1e3 / r['ms_per_step'], rel=1e-9)
    assert r['roofline']['launches'] == r['roofline']['launches_expected'] == 11 * 3
    for k in ('parity', 'cpu_baseline', 'per_config', 'f16_fast_path', 'fp32_exact_path'):
        assert k not in r, k
    assert r['roofline']['achieved_isolated'] is None


def test_dump_holds_the_last_steps_outputs(plain_run, dev):
    import bench
    _, d = plain_run
    got = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    assert set(got) == {f'{m}_{n}' for m, names in bench.OUT_NAMES.items() for n in names} | {'rows'}
    assert all(v.dtype == np.float32 and v.shape[0] == B and np.isfinite(v).all() for v in got.values())
    rows = np.concatenate([got['speech_probs'], got['text_probs'], got['image_probs'], got['fusion_probs'],
                           got['fusion_attention_weights'], got['fusion_decision_weights']], axis=1)
    assert got['rows'].shape == (B, bench.ROW) and np.array_equal(got['rows'], rows)
    # the bench's seeded inputs and weights through a pipeline of this process: the same probabilities.
    # GEMM tiles are autotuned per process, so not bit for bit: the fp32x3 path is held to 1e-5 on probs
    # against the oracle (test_gpu_fp32x3.py), hence two runs of it to 2e-5 against each other
    pipe = engine.FusedPipeline(seed=1234, device=dev, precision='fp32x3')
    args = [engine.to_device(a, dev) for a in (syn.speech_inputs(B, seed=0), *syn.text_inputs(B, 128, seed=0, ragged=False),
                                               syn.image_inputs(B, seed=0))]
    out = pipe.forward(*args)
    pipe.wait()
    pipe.check()
    for mod, names in bench.OUT_NAMES.items():
        for n, t in zip(names, out[mod]):
            if n == 'probs':
                err = float(np.abs(got[f'{mod}_{n}'] - t.cpu().numpy()).max())
                print(f'  {mod} probs, bench dump vs this process: max|d| {err:.3g}')
                assert err <= 2e-5, (mod, err)
    for m in pipe.models():
        m.close()
