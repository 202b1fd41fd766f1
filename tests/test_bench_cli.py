"""bench.py's command line: --dump-outputs and what a plain run leaves to --full.

The dump holds what the last timed step returned (loss, log_z, num, dW) as
float32 .npy files, at most 64 MB in all, a fixed seeded sample of an array
too large for that. The GPU test runs one small plain benchmark and checks
the dumped arrays against the oracle on the inputs bench.py generates.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from golden_cases import assert_grad_marginal_close, assert_loss_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the legs of a --full run: none of them may appear in a plain run's line
FULL_KEYS = ('north_star_b256', 'realistic_weights', 'cold_w', 'joint_weight_fn_step',
             'cpu_baseline', 'cpu_baseline_torch', 'cpu_baseline_oracle')


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
  import bench
  # the sampled arrays' budget and three whole ones of at most 1 MB each
  assert bench.DUMP_BUDGET_BYTES + 3 * 1000 * 1000 <= 64 * 1000 * 1000
  monkeypatch.setattr(bench, 'DUMP_BUDGET_BYTES', 2 * 1000 * 1000)  # a quick test
  g = torch.Generator().manual_seed(3)
  small = torch.randn([7], generator=g, dtype=torch.float64)
  n_big = bench.DUMP_BUDGET_BYTES // 4 + 1001  # just over its share: sampled
  big = torch.arange(n_big, dtype=torch.float32).reshape(1, 1, -1)
  bench.dump_outputs({'loss': small, 'dW': big}, str(tmp_path / 'a'))
  bench.dump_outputs({'loss': small, 'dW': big}, str(tmp_path / 'b'))
  a = {k: np.load(tmp_path / 'a' / f'{k}.npy') for k in ('loss', 'dW')}
  b = {k: np.load(tmp_path / 'b' / f'{k}.npy') for k in ('loss', 'dW')}
  assert sorted(os.listdir(tmp_path / 'a')) == ['dW.npy', 'loss.npy']
  for k in a:
    assert a[k].dtype == np.float32
    np.testing.assert_array_equal(a[k], b[k])  # the same sample every time
  np.testing.assert_array_equal(a['loss'], small.float().numpy())  # whole, its shape kept
  # the sample: values of big are their own flat indices, so they are in
  # range, sorted, and spread over the array
  s = a['dW']
  assert s.shape == (bench.DUMP_BUDGET_BYTES // 4,)
  assert (np.diff(s) >= 0).all() and s[0] >= 0 and s[-1] < n_big
  assert s[0] < n_big // 100 and s[-1] > n_big - n_big // 100
  total = sum(os.path.getsize(tmp_path / 'a' / f) for f in os.listdir(tmp_path / 'a'))
  assert total <= bench.DUMP_BUDGET_BYTES + 3 * 1000 * 1000


@pytest.mark.gpu
def test_plain_run_dumps_the_timed_outputs(cuda, tmp_path):
  from oracle import oracle as orc
  import bench
  B, T, U, V, n = 3, 50, 6, 8, 1
  out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps',
                        '3', '--warmup', '1', '--batch', str(B), '--frames', str(T), '--labels',
                        str(U), '--vocab', str(V), '--context', str(n), '--dump-outputs',
                        str(tmp_path)], capture_output=True, text=True, timeout=120, cwd=ROOT)
  assert out.returncode == 0, out.stderr[-2000:]
  line = [x for x in out.stdout.splitlines() if x.startswith('{')]
  assert len(line) == 1, out.stdout
  r = json.loads(line[0])
  assert r['steps'] == 3 and r['warmup'] == 1 and r['unit'] == 'cells/s' and r['dtype'] == 'f32'
  assert r['higher_is_better'] is True and r['ms_per_step'] > 0
  np.testing.assert_allclose(r['value'], B * T * U * (V + 1) / (r['ms_per_step'] * 1e-3),
                             rtol=1e-9)
  assert not [k for k in FULL_KEYS if k in r]
  # bench.py's inputs, regenerated, through the oracle
  nf, lab, nl = bench.global_batch(B, T, U, V, 1234, False)
  W = bench.shard_weights(range(B), T, V + 1, V, cuda, 1234).cpu().numpy()
  rl, rlz, rnum, rdW = orc.loss_grad(W, nf.numpy(), lab.numpy(), nl.numpy(), V, n)
  den = orc.den_grad(W, nf.numpy(), V, n)[1]
  got = {k: np.load(tmp_path / f'{k}.npy') for k in ('loss', 'log_z', 'num', 'dW')}
  assert all(x.dtype == np.float32 for x in got.values())
  assert_loss_close(got['loss'], rl)
  assert_loss_close(got['log_z'], rlz)
  assert_loss_close(got['num'], rnum)
  assert got['dW'].shape == rdW.shape
  assert_grad_marginal_close(got['dW'], rdW, den, rlz, rnum)
