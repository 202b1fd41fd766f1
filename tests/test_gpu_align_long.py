"""Forced alignment of long label strings on the GPU (RecognitionLattice.align
-> lt_table_align_long, lt_align_long.hip; 256 <= U <= 4095): all three
outputs exact against the pinned C oracle (table_oracle.c tab_dist_grad in
MaxTropical, compacted by align_compact.compact), with integer weights (ties in
almost every cell) and Gaussian ones. V = 4 bigram and T = U + 7 unless noted:
every path runs along the diagonal and crosses every wave boundary.
"""
import zlib

import numpy as np
import pytest
import torch

import last_torch_amd as lt
from last_torch_amd import _native as nat
from align_compact import compact
import poisoned_buffers
from test_gpu_align import _align, _assert_equal, _lattice, _lengths, _weights

pytestmark = pytest.mark.gpu

CHUNK = 256  # kChunk of lt_align_long.hip: frames the backtrace stages at a time

CASES = {
    # name: V, C (random table) or None (bigram), U, T, dtype, epsilons
    'u256': (4, None, 256, 263, 'f32', False),   # the first position of a second wave
    'u511': (4, None, 511, 518, 'f32', False),
    'u512': (4, None, 512, 519, 'f32', False),
    'u767': (4, None, 767, 774, 'f32', False),
    'u1023': (4, None, 1023, 1030, 'f32', False),
    'u1024': (4, None, 1024, 1031, 'f32', False),  # the first 5-wave string
    'u2047': (4, None, 2047, 2054, 'f32', False),  # 8 waves: the deep weight ring's last
    'u2048': (4, None, 2048, 2055, 'f32', False),  # 9 waves: the short ring's first
    'u4095': (4, None, 4095, 4102, 'f32', False),  # 16 waves
    'u300_t700': (4, None, 300, 700, 'f32', False),  # slack: long blank runs inside a wave
    'bf16_u512': (4, None, 512, 519, 'bf16', False),
    'table_c300_v28_u300_eps': (28, 300, 300, 320, 'f32', True),  # too large to stage in LDS
    # nf around the pipeline's 16-frame blocks, strings of one wave (nl <= 255: the others only
    # pass the barriers) to three, and 607 frames of decisions: three staging chunks of CHUNK
    'ragged_u600': (4, None, 600, 2 * CHUNK + 95, 'f32', False),
}
RAGGED_NF = [1, 15, 16, 17, 33, 607, 607, 607]
RAGGED_NL = [1, 15, 10, 17, 33, 600, 597, 200]
_PROBLEMS = {}


def _problem(name, kind, variant=''):
  """The problem and its reference, computed once and changed by nothing."""
  key = f'{name}-{kind}{variant}'
  if key not in _PROBLEMS:
    from oracle import oracle as orc  # test infrastructure only
    V, C, U, T, dt, eps = CASES[name]
    rng = np.random.default_rng(zlib.crc32(key.encode()))
    if C is None:
      ctx, tab = lt.contexts.FullNGram(vocab_size=V, context_size=1), orc.full_ngram_table(V, 1)
    else:
      tab = rng.integers(0, C, (C, V)).astype(np.int32)
      ctx = lt.contexts.NextStateTable(torch.tensor(tab))
    if name.startswith('ragged'):
      nf, nl = np.array(RAGGED_NF, np.int32), np.array(RAGGED_NL, np.int32)
    else:
      nf, nl = _lengths(rng, T, U, 0)
    W = _weights(rng, kind, (len(nf), T, tab.shape[0], V + 1))
    if dt == 'bf16':
      W = torch.tensor(W).bfloat16().float().numpy()
    lab = rng.integers(0 if eps else 1, V + 1, (len(nf), U)).astype(np.int32)
    rd, rg = orc.tab_dist_grad(tab, W, nf, 0, orc.MAX, lab, nl)
    ref = compact(rg, rd, lab, nl, nf, 0) + (rd,)
    if name.startswith('ragged'):
      assert np.isfinite(rd).all()
    else:
      assert np.isfinite(rd[:3]).all() and rd[3] == -np.inf and (ref[1][3] == -1).all()
    _PROBLEMS[key] = (ctx, W, nf, lab, nl, dt, ref)
  return _PROBLEMS[key]


def _direct(lat, W, nf, lab, nl, dev, fn=None, dt='f32'):
  """fn (default: the binding's table_align_long) on ROCm tensors, as numpy."""
  Wd = torch.tensor(W, device=dev)
  out = (fn or nat.table_align_long)(
      lat._graph(dev), Wd.bfloat16().contiguous() if dt == 'bf16' else Wd,
      torch.tensor(nf, device=dev), torch.tensor(lab, device=dev), torch.tensor(nl, device=dev))
  return [x.cpu().numpy() for x in out]


@pytest.mark.parametrize('name', list(CASES))
@pytest.mark.parametrize('kind', ['ints', 'gauss'])
def test_long_align_against_oracle(cuda, name, kind):
  ctx, W, nf, lab, nl, dt, ref = _problem(name, kind)
  Wd = torch.tensor(W, device=cuda)
  lat = _lattice(ctx, 0, Wd)
  graph, labd = lat._graph(cuda), torch.tensor(lab, device=cuda)
  assert not nat.table_align_supported(graph, Wd, labd)
  assert nat.table_align_long_supported(graph, Wd, labd)
  _assert_equal(_direct(lat, W, nf, lab, nl, cuda, dt=dt), *ref)
  _assert_equal(_align(lat, W, nf, lab, nl, cuda), *ref)  # fp32: the widened values for bf16


def test_long_align_poisoned_and_stale_memory(cuda, monkeypatch):
  """Outputs and workspace prefilled with 0xA5 bytes, then as a finished call
  on another problem left them: the reference both times, and a third run is
  bit-equal to the first."""
  ctx, W, nf, lab, nl, _, ref = _problem('ragged_u600', 'ints')
  _, W2, nf2, lab2, nl2, _, _ = _problem('ragged_u600', 'gauss', '-other')
  lat = _lattice(ctx, 0, torch.tensor(W, device=cuda))
  monkeypatch.setattr(poisoned_buffers, 'POISON_BYTE', 0xA5)
  with poisoned_buffers.poisoned(nat):
    first = _direct(lat, W, nf, lab, nl, cuda)
  _assert_equal(first, *ref)
  with poisoned_buffers.stale(nat) as s:
    s.record(_direct, lat, W2, nf2[::-1].copy(), lab2, nl2[::-1].copy(), cuda)
    _assert_equal(s.replay(_direct, lat, W, nf, lab, nl, cuda), *ref)
  for x, y in zip(_direct(lat, W, nf, lab, nl, cuda), first):
    np.testing.assert_array_equal(x, y)


def test_long_align_dense_route_agrees(cuda):
  """_align_dense, the fallback past U = 4095 and the timing baseline, gives
  the kernel's three outputs exactly."""
  ctx, W, nf, lab, nl, _, ref = _problem('u300_t700', 'ints')
  lat = _lattice(ctx, 0, torch.tensor(W, device=cuda))
  dense = _direct(lat, W, nf, lab, nl, cuda, fn=lat._align_dense)
  _assert_equal(dense, *ref)
  for x, y in zip(_direct(lat, W, nf, lab, nl, cuda), dense):
    np.testing.assert_array_equal(x, y)
