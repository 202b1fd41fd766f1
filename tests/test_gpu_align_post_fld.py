"""Emission posteriors on FrameLabelDependent(K) on the GPU
(RecognitionLattice.align_posteriors -> lt_table_align_posteriors_fld,
lt_align_post_fld.hip; 1 <= K <= 15, U <= 255) against the float64 reference
of tests/align_post_ref.py: K = 1, the lane and slice boundaries with nearly
every frame emitting K labels, T > U (the history in the workspace), K = 15 at
P = 1 and P = 4, K > U, epsilons, a table too large to stage, bf16, -inf arcs,
the ring and midpoint boundaries, and poisoned and stale memory.

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
from test_gpu_align_post import _check, _frames, _lattice, _lengths

pytestmark = pytest.mark.gpu

CASES = [
    # name, V, n (FullNGram) or None (random table of C states), C, K, T, U, dtype, epsilon, -inf
    ('fld1_u9', 4, 1, None, 1, 14, 9, 'f32', False, False),  # K = 1: the blank is mandatory
    ('fld2_u63', 8, 1, None, 2, 36, 63, 'f32', False, False),  # T K barely >= U
    ('fld2_u64', 8, 1, None, 2, 36, 64, 'f32', False, False),  # P 1 -> 2
    ('fld2_u65', 8, 1, None, 2, 37, 65, 'f32', False, False),
    ('fld3_u127', 8, 1, None, 3, 46, 127, 'f32', False, False),
    ('fld3_u128', 8, 1, None, 3, 46, 128, 'f32', False, False),  # P 2 -> 4
    ('fld3_u255', 8, 1, None, 3, 89, 255, 'f32', False, False),  # last position of the range
    # 76 rows of 8 * 256 bytes fit LDS beside the prologue's arrays: the history in the workspace
    ('fld2_u130_t140', 8, 1, None, 2, 140, 130, 'f32', False, False),
    ('fld15_u50_t6', 4, 1, None, 15, 6, 50, 'f32', False, False),  # the chain crosses 15 lanes
    ('fld15_u200_t17', 4, 1, None, 15, 17, 200, 'f32', False, False),  # K = 15 at P = 4
    ('fld2_trigram_eps', 5, 2, None, 2, 12, 9, 'f32', True, False),
    ('fld2_table_c300_v28_t20', 28, None, 300, 2, 20, 9, 'f32', True, False),  # table not staged
    ('fld2_bf16_u65', 8, 1, None, 2, 37, 65, 'bf16', False, False),
    ('fld2_v4_minus_inf', 4, 1, None, 2, 30, 9, 'f32', False, True),
    ('fld5_u3', 4, 1, None, 5, 8, 3, 'f32', False, False),  # K > U: three frames take all U labels
]
_BY_NAME = {c[0]: c for c in CASES}
_PROBLEMS = {}


def _problem(name, variant=''):
  """test_gpu_align_post._problem's recipe on FrameLabelDependent(K); computed
  once, changed by nothing."""
  key = name + variant
  if key not in _PROBLEMS:
    _, V, n, C, K, T, U, dt, eps, minf = _BY_NAME[name]
    rng = np.random.default_rng(zlib.crc32(key.encode()))
    if n is not None:
      ctx = lt.contexts.FullNGram(vocab_size=V, context_size=n)
    else:
      ctx = lt.contexts.NextStateTable(torch.tensor(rng.integers(0, C, (C, V)).astype(np.int32)))
    W = rng.standard_normal((4, T, ctx.shape()[0], V + 1)).astype(np.float32)
    if minf:
      W[rng.random(W.shape) < 0.05] = -np.inf
    W = torch.tensor(W)
    if dt == 'bf16':
      W = W.bfloat16().float()
    if K <= U:
      nf, nl = _lengths(rng, T, U, K)
    else:  # _lengths' numbers where its fourth utterance (three frames, U labels) is aligned
      nf = np.array([T, T, 0, 3], np.int32)
      nl = np.array([U, U - int(rng.integers(0, 4)), 0, U], np.int32)
    lab = rng.integers(0 if eps else 1, V + 1, (4, U)).astype(np.int32)
    nf, nl, lab = torch.tensor(nf), torch.tensor(nl), torch.tensor(lab)
    e_err, l_err, e64, l64 = yardstick(W, nf, lab, nl, ctx, K)
    assert torch.isfinite(l64[:2]).all() and l64[2] == 0
    assert torch.isfinite(l64[3]) if K > U else l64[3] == -torch.inf
    _PROBLEMS[key] = (ctx, K, W, nf, lab, nl, dt, e_err, l_err, e64, l64)
  return _PROBLEMS[key]


def _run(ctx, K, W, nf, lab, nl, dt, device):
  """(emission, log_prob): fp32 through the public method, bf16 (TableWeightFn
  hands out fp32) through the binding; the old kernel refuses either."""
  Wd, nfd, labd, nld = W.to(device), nf.to(device), lab.to(device), nl.to(device)
  lat = _lattice(ctx, K, Wd)
  graph = lat._graph(device)
  assert nat.table_align_posteriors_fld_supported(graph, Wd, labd)
  assert not nat.table_align_posteriors_supported(graph, Wd, labd)
  if dt == 'bf16':
    return nat.table_align_posteriors_fld(graph, Wd.bfloat16().contiguous(), nfd, labd, nld)
  return lat.align_posteriors(_frames(tuple(nf.shape), W.shape[1], device), nfd, labd, nld)


@pytest.mark.parametrize('name', [c[0] for c in CASES])
def test_fld_align_posteriors_match_reference(cuda, name):
  ctx, K, W, nf, lab, nl, dt, e_err, l_err, e64, l64 = _problem(name)
  em, lp = _run(ctx, K, W, nf, lab, nl, dt, cuda)
  _check(name, em, lp, None, nf, nl, e_err, l_err, e64, l64)


def test_fld_ring_and_midpoint_boundaries(cuda):
  """num_frames 1, 2, 3, 15, 16, 17, 33 in one batch at U = 9, K = 2: odd and
  even midpoints, phases shorter than, equal to and one past the 16-frame
  ring; the three shortest utterances need two labels on a frame."""
  V, T, U, K = 6, 33, 9, 2
  rng = np.random.default_rng(33)
  ctx = lt.contexts.FullNGram(vocab_size=V, context_size=1)
  W = torch.tensor(rng.standard_normal((7, T, ctx.num_states(), V + 1)).astype(np.float32))
  nf = torch.tensor([1, 2, 3, 15, 16, 17, 33], dtype=torch.int32)
  nl = torch.tensor([2, 4, 5, 9, 9, 8, 9], dtype=torch.int32)
  lab = torch.tensor(rng.integers(1, V + 1, (7, U)).astype(np.int32))
  e_err, l_err, e64, l64 = yardstick(W, nf, lab, nl, ctx, K)
  assert torch.isfinite(l64).all()
  em, lp = _run(ctx, K, W, nf, lab, nl, 'f32', cuda)
  _check('fld_ring_midpoint', em, lp, None, nf, nl, e_err, l_err, e64, l64)


def test_fld_poisoned_and_stale_buffers_and_determinism(cuda):
  """Every output and workspace byte is the call's own: the results on 0xFF
  memory, and on the memory a finished call on another problem of the same
  shape left behind, are bit-equal to a plain run; so are two plain runs and
  the public method's result."""
  ctx, K, W, nf, lab, nl, *_ = _problem('fld2_u130_t140')
  _, _, W2, nf2, lab2, nl2, *_ = _problem('fld2_u130_t140', '-other')
  lat = _lattice(ctx, K, W.to(cuda))
  graph = lat._graph(cuda)

  def call(W_, nf_, lab_, nl_):
    return nat.table_align_posteriors_fld(graph, W_.to(cuda), nf_.to(cuda), lab_.to(cuda),
                                          nl_.to(cuda))

  nbytes = nat.ctypes.c_size_t(0)
  pb = nat._tproblem(graph, W.to(cuda), lab.shape[-1])
  nat._check(nat.lib().lt_table_align_posteriors_fld_workspace_bytes(
      nat.ctypes.byref(graph.g), nat.ctypes.byref(pb), nat.ctypes.byref(nbytes)), 'query')
  assert nbytes.value > 0  # the workspace path
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
