"""bench.py's plain run and --dump-outputs: the dump helper on CPU tensors
(whole batch below the sample limit, a fixed seeded sample above it), and one
small GPU run whose dumped batch equals the same call made through the API
and whose line carries the headline alone."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

BENCH = os.path.join(REPO, 'bench.py')


def _bench_mod():
    spec = importlib.util.spec_from_file_location('bench_mod_outputs', BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_whole_batch_below_the_limit(tmp_path):
    import torch
    bench = _bench_mod()
    buf = (torch.arange(3 * 96, dtype=torch.int32) % 1024).to(torch.int16).reshape(3, 96)
    bench.dump_outputs(str(tmp_path / 'd'), buf, 0)
    got = np.load(tmp_path / 'd' / 'sdr.npy')
    assert got.dtype == np.float32 and got.shape == (3, 96)
    assert np.array_equal(got, buf.numpy().astype(np.float32))


def test_dump_samples_a_large_batch_at_fixed_positions(tmp_path, monkeypatch):
    import torch
    bench = _bench_mod()
    assert bench.DUMP_MAX_SAMPLES * 4 <= 64 * 1000 * 1000        # float32 dump stays under 64 MB
    monkeypatch.setattr(bench, 'DUMP_MAX_SAMPLES', 128)
    buf = (torch.arange(5 * 1000, dtype=torch.int32) % 251).to(torch.uint8).reshape(5, 1000)
    bench.dump_outputs(str(tmp_path), buf, 0)
    bench.dump_outputs(str(tmp_path), buf, 1)                    # another rank: its own file, same positions
    a, b = np.load(tmp_path / 'sdr.npy'), np.load(tmp_path / 'sdr_rank1.npy')
    assert a.dtype == np.float32 and a.shape == (128,) and np.array_equal(a, b)
    idx = np.sort(np.random.RandomState(bench.DUMP_SEED).randint(0, 5000, size=128, dtype=np.int64))
    assert np.array_equal(a, buf.numpy().reshape(-1)[idx].astype(np.float32))
    # a changed sample shows: the positions cover the batch, not its head alone
    assert idx[0] < 1000 and idx[-1] >= 4000


def test_full_is_off_by_default(monkeypatch):
    bench = _bench_mod()
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '3', '--warmup', '1'])
    args = bench.parse_args()
    assert args.full is False and args.dump_outputs is None and args.steps == 3
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--full', '--dump-outputs', 'x'])
    args = bench.parse_args()
    assert args.full is True and args.dump_outputs == 'x'


@pytest.mark.gpu
def test_plain_run_dumps_what_the_api_returns(tmp_path):
    """One small plain run (2 frames of 256x128): the line holds the headline
    fields and none of the --full sections, and sdr.npy is the output batch of
    the same h2s_process call on the same seeded frames, sample for sample."""
    import torch

    import hdr2sdr
    from hdr2sdr.synth import synth_frames
    W, H, B = 256, 128, 2
    out = subprocess.run([sys.executable, BENCH, '--gpus', '1', '--steps', '2', '--warmup', '1', '--frames', str(B),
                          '--width', str(W), '--height', str(H), '--dump-outputs', str(tmp_path)],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1
    rec = lines[0]
    assert rec['steps'] == 2 and rec['warmup'] == 1 and rec['ms_per_step'] > 0
    assert rec['unit'] == 'Mpixel/s' and rec['higher_is_better'] is True and rec['dtype'] == 'f32'
    assert abs(rec['value'] - B * W * H / (rec['ms_per_step'] * 1e-3) / 1e6) <= 0.01 * rec['value'] + 0.1
    c = rec['config']
    assert c['alt_content'] is None and c['real_content'] is None and c['other_configs'] is None
    assert c['host_path'] is None and c['sharded_configs'] == {} and rec['cpu_baseline'] is None

    got = np.load(tmp_path / 'sdr.npy')
    assert got.dtype == np.float32 and got.shape == (B, W * H * 3 // 2)
    params = hdr2sdr.TonemapParams(tonemapper='hable', gamma=2.2, bits_in=10, bits_out=10)
    tm = hdr2sdr.Tonemapper(0, params, hdr2sdr.generate_lattice(65))
    src = synth_frames('smooth', B, W, H, 10, device='cuda:0', seed=0x5EED)
    want = tm(src)
    torch.cuda.synchronize()
    tm.close()
    assert np.array_equal(got, want.to_numpy().buf.astype(np.float32))
