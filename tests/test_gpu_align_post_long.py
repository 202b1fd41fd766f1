"""Emission posteriors of long label strings on the GPU
(RecognitionLattice.align_posteriors -> lt_table_align_posteriors_long,
lt_align_post_long.hip; 256 <= U <= 1023) against the float64 reference of
tests/align_post_ref.py: at the wave counts' boundaries with the posterior
mass crossing every wave boundary (T = U + 7), bf16, a table too large to
stage with epsilons, -inf arcs, the pipeline's block boundaries, and on
poisoned and stale memory.

Bounds: test_gpu_align_post.py's (its _check): at most 4x the float32
yardstick's error on emission and log_prob, column sums off 1 by at most that
bound x T; every figure is printed before it is asserted (pytest -s).
DESIGN.md section 3k lists the measured figures.
"""
import zlib

import numpy as np
import pytest
import torch

import last_torch_amd as lt
from last_torch_amd import _native as nat
from align_post_ref import yardstick
import poisoned_buffers
from test_gpu_align_post import _check, _frames, _lattice

pytestmark = pytest.mark.gpu

F = 16  # kLongF of lt_align_post_long.hip: frames of a pipeline block

CASES = [
    # name, V, C (random table) or None (bigram), U, dtype, epsilon, -inf, T - U. T = U + 7: the
    # only paths run near the diagonal and the posterior mass crosses every wave boundary
    ('u256', 4, None, 256, 'f32', False, False, 7),   # the first position of a second wave
    ('u511', 4, None, 511, 'f32', False, False, 7),
    ('u512', 4, None, 512, 'f32', False, False, 7),   # NW 2 -> 3
    ('u767', 4, None, 767, 'f32', False, False, 7),
    ('u768', 4, None, 768, 'f32', False, False, 7),   # NW 3 -> 4
    ('u1023', 4, None, 1023, 'f32', False, False, 7),
    ('bf16_u512', 4, None, 512, 'bf16', False, False, 7),
    ('table_c300_v28_u300_eps', 28, 300, 300, 'f32', True, False, 7),  # too large to stage in LDS
    # 5 % -inf arcs leave no path through a band of 8 frames over 300 labels: 41 frames of slack
    ('minus_inf_u300', 4, None, 300, 'f32', False, True, 40),
    ('u300', 4, None, 300, 'f32', False, False, 7),   # the hygiene test's
]
_BY_NAME = {c[0]: c for c in CASES}
_PROBLEMS = {}


def _problem(name, variant=''):
  """test_gpu_align_post._problem's recipe: four utterances (full length, a
  little shorter, empty, three frames with one label too many), N(0, 1)
  weights, seeded from the name; computed once, changed by nothing."""
  key = name + variant
  if key not in _PROBLEMS:
    _, V, C, U, dt, eps, minf, slack = _BY_NAME[name]
    T = U + slack
    rng = np.random.default_rng(zlib.crc32(key.encode()))
    if C is None:
      ctx = lt.contexts.FullNGram(vocab_size=V, context_size=1)
    else:
      ctx = lt.contexts.NextStateTable(torch.tensor(rng.integers(0, C, (C, V)).astype(np.int32)))
    W = rng.standard_normal((4, T, ctx.shape()[0], V + 1)).astype(np.float32)
    if minf:
      W[rng.random(W.shape) < 0.05] = -np.inf
    W = torch.tensor(W)
    if dt == 'bf16':
      W = W.bfloat16().float()
    nf = torch.tensor([T, T, 0, 3], dtype=torch.int32)
    nl = torch.tensor([U, U - 2, 0, 4], dtype=torch.int32)
    lab = torch.tensor(rng.integers(0 if eps else 1, V + 1, (4, U)).astype(np.int32))
    e_err, l_err, e64, l64 = yardstick(W, nf, lab, nl, ctx)
    # the reference alone leaves only the short utterance unaligned
    assert torch.isfinite(l64[:3]).all() and l64[3] == -torch.inf and l64[2] == 0
    _PROBLEMS[key] = (ctx, W, nf, lab, nl, dt, e_err, l_err, e64, l64)
  return _PROBLEMS[key]


@pytest.mark.parametrize('name', [c[0] for c in CASES[:-1]])
def test_long_align_posteriors_match_reference(cuda, name):
  ctx, W, nf, lab, nl, dt, e_err, l_err, e64, l64 = _problem(name)
  Wd, nfd, labd, nld = W.to(cuda), nf.to(cuda), lab.to(cuda), nl.to(cuda)
  lat = _lattice(ctx, 0, Wd)
  graph = lat._graph(cuda)
  assert nat.table_align_posteriors_long_supported(graph, Wd, labd)
  assert not nat.table_align_posteriors_supported(graph, Wd, labd)
  if dt == 'bf16':  # TableWeightFn hands out fp32: the bf16 kernel through the binding
    em, lp = nat.table_align_posteriors_long(graph, Wd.bfloat16().contiguous(), nfd, labd, nld)
  else:
    em, lp = lat.align_posteriors(_frames((4,), W.shape[1], cuda), nfd, labd, nld)
  _check(name, em, lp, None, nf, nl, e_err, l_err, e64, l64)


def test_pipeline_block_boundaries(cuda):
  """num_frames 1, 2, F-1, F, F+1, 2F, 2F+1, 4F+3 in one batch at max_labels =
  300 (two waves a direction): odd and even midpoints, phases shorter than one
  block, blocks shorter than the skew, drain and refill with no full block."""
  V, U = 4, 300
  nf = torch.tensor([1, 2, F - 1, F, F + 1, 2 * F, 2 * F + 1, 4 * F + 3], dtype=torch.int32)
  nl = torch.tensor([1, 2, F - 1, F - 3, F + 1, 2 * F, 2 * F - 5, 4 * F + 3], dtype=torch.int32)
  B, T = len(nf), int(nf.max())
  rng = np.random.default_rng(4 * F + 3)
  ctx = lt.contexts.FullNGram(vocab_size=V, context_size=1)
  W = torch.tensor(rng.standard_normal((B, T, ctx.num_states(), V + 1)).astype(np.float32))
  lab = torch.tensor(rng.integers(1, V + 1, (B, U)).astype(np.int32))
  e_err, l_err, e64, l64 = yardstick(W, nf, lab, nl, ctx)
  assert torch.isfinite(l64).all()
  lat = _lattice(ctx, 0, W.to(cuda))
  assert nat.table_align_posteriors_long_supported(lat._graph(cuda), W.to(cuda), lab.to(cuda))
  em, lp = lat.align_posteriors(_frames((B,), T, cuda), nf.to(cuda), lab.to(cuda), nl.to(cuda))
  _check('block_boundaries', em, lp, None, nf, nl, e_err, l_err, e64, l64)


def test_long_poisoned_and_stale_buffers_and_determinism(cuda):
  """Every output and workspace byte is the call's own: the results on 0xFF
  memory, and on the memory a finished call on another problem of the same
  shape left behind, are bit-equal to a plain run; so are two plain runs."""
  ctx, W, nf, lab, nl, *_ = _problem('u300')
  _, W2, nf2, lab2, nl2, *_ = _problem('u300', '-other')
  lat = _lattice(ctx, 0, W.to(cuda))
  graph = lat._graph(cuda)

  def call(W_, nf_, lab_, nl_):
    return nat.table_align_posteriors_long(graph, W_.to(cuda), nf_.to(cuda), lab_.to(cuda),
                                           nl_.to(cuda))

  plain = [x.clone() for x in call(W, nf, lab, nl)]
  again = call(W, nf, lab, nl)
  assert torch.equal(plain[0], again[0]) and torch.equal(plain[1], again[1])
  with poisoned_buffers.poisoned(nat):
    got = call(W, nf, lab, nl)
    frames = _frames((4,), W.shape[1], cuda)
    whole = lat.align_posteriors(frames, nf.to(cuda), lab.to(cuda), nl.to(cuda))
  assert torch.equal(plain[0], got[0]) and torch.equal(plain[1], got[1])
  assert torch.equal(plain[0], whole[0]) and torch.equal(plain[1], whole[1])
  with poisoned_buffers.stale(nat) as s:
    s.record(call, W2, nf2, lab2, nl2)
    got = s.replay(call, W, nf, lab, nl)
    assert torch.equal(plain[0], got[0]) and torch.equal(plain[1], got[1])
