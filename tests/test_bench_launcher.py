"""CPU: bench.py's multi-GPU launcher and sharding, without a GPU.

`python bench.py --gpus N` with no WORLD_SIZE starts N ranks through torch.distributed.run as a
child process (before any GPU call); with no GPU visible each rank runs the stub step over gloo:
the same sharding (mec.dist.shard), all-gather (mec.dist.all_gather_rows) and max-over-ranks
timing as the GPU run, on deterministic stand-in rows. The JSON line must report N ranks as
torch.distributed saw them and the gathered rows in global sample order."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(*args, timeout=240):
    env = dict(os.environ, CUDA_VISIBLE_DEVICES='', HIP_VISIBLE_DEVICES='', OMP_NUM_THREADS='1')
    env.pop('WORLD_SIZE', None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), *args], capture_output=True, text=True,
                       timeout=timeout, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, p.stdout[-2000:]  # rank 0 prints ONE line
    return json.loads(lines[0])


@pytest.mark.parametrize('n', [2, 3])
def test_bench_gpus_n_launches_n_ranks(n):
    r = _run_bench('--gpus', str(n), '--steps', '2', '--warmup', '1', '--batch', '5')
    assert r['n_gpus'] == n and r['stub'] is True and r['value'] is None
    d = r['distributed']
    assert d['world_size'] == n and d['backend'] == 'gloo'
    assert d['gathered_rows_in_order'] is True
    assert r['config']['global_batch'] == 5 * n and r['scaling'] == 'weak'


def test_bench_single_rank_stub():
    r = _run_bench('--steps', '1', '--warmup', '0')
    assert r['n_gpus'] == 1 and r['distributed']['gathered_rows_in_order'] is True


def test_bench_stub_dumps_the_gathered_rows(tmp_path):
    """--dump-outputs DIR: the rows the last step produced, float32, a function of the arguments alone."""
    sys.path.insert(0, ROOT)
    import bench
    r = _run_bench('--gpus', '2', '--steps', '2', '--warmup', '1', '--batch', '5', '--dump-outputs', str(tmp_path / 'a'))
    assert r['steps'] == 2 and r['ms_per_step'] > 0
    a = np.load(tmp_path / 'a' / 'rows.npy')
    assert os.listdir(tmp_path / 'a') == ['rows.npy'] and a.dtype == np.float32 and a.shape == (10, bench.ROW)
    assert np.array_equal(a, bench.stub_rows(0, 10).numpy())


def test_dump_outputs_names_dtype_and_size_cap(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    import torch
    B = 64
    rng = np.random.default_rng(0)
    out = {mod: tuple(torch.from_numpy(rng.standard_normal((B, 7 + i)).astype(np.float32)) for i in range(len(names)))
           for mod, names in bench.OUT_NAMES.items()}
    rows = torch.from_numpy(rng.standard_normal((2 * B, bench.ROW)))  # float64 in, gathered over 2 ranks
    bench.dump_outputs(str(tmp_path / 'all'), out, rows)
    want = {f'{m}_{n}.npy' for m, names in bench.OUT_NAMES.items() for n in names} | {'rows.npy'}
    assert set(os.listdir(tmp_path / 'all')) == want
    for f in want:
        assert np.load(tmp_path / 'all' / f).dtype == np.float32
    assert np.array_equal(np.load(tmp_path / 'all' / 'text_probs.npy'), out['text'][2].numpy())
    assert np.array_equal(np.load(tmp_path / 'all' / 'rows.npy'), rows.numpy().astype(np.float32))
    # over the cap: every array keeps the same seeded sample size of its rows, and the total fits
    monkeypatch.setattr(bench, 'DUMP_BYTES', 4096)
    for d in ('c1', 'c2'):
        bench.dump_outputs(str(tmp_path / d), out, rows)
    got = {f: np.load(tmp_path / 'c1' / f) for f in want}
    assert sum(v.nbytes for v in got.values()) <= 4096 and len({len(v) for v in got.values()}) == 1
    assert all(np.array_equal(v, np.load(tmp_path / 'c2' / f)) for f, v in got.items())
    full = out['image'][0].numpy()
    assert all(any(np.array_equal(r, f) for f in full) for r in got['image_feat.npy'])


def test_plain_run_times_the_headline_precision_only():
    sys.path.insert(0, ROOT)
    import bench
    assert bench.headline_precision('all') == (['f16', 'fp32x3', 'fp32'], 'fp32x3')
    assert bench.headline_precision('both') == (['f16', 'fp32'], 'fp32')
    assert bench.headline_precision('f16') == (['f16'], 'f16')
    a = bench.parse([])
    assert a.full is False and a.dump_outputs is None
    assert bench.parse(['--full', '--dump-outputs', 'd']).full is True


def test_stub_rows_and_shards_tile_the_global_batch():
    sys.path.insert(0, ROOT)
    import bench
    from mec import dist as mdist
    world, B = 4, 7
    parts = [bench.stub_rows(*mdist.shard(world * B, world, r)) for r in range(world)]
    full = bench.stub_rows(0, world * B)
    assert np.array_equal(np.concatenate([p.numpy() for p in parts]), full.numpy())


@pytest.mark.parametrize('B', [256, 1024, 300])
def test_parity_rows_cover_every_quarter(B):
    sys.path.insert(0, ROOT)
    import bench
    rows = bench.parity_rows(B, 256)
    if B <= 256:
        assert rows == list(range(B))
        return
    assert rows == sorted(set(rows)) and rows[0] == 0 and rows[-1] == B - 1
    for q in range(4):
        lo, hi = q * B // 4, (q + 1) * B // 4
        assert sum(lo <= r < hi for r in rows) >= 4, (q, rows)
    assert any(r >= 256 for r in rows)
