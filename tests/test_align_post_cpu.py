"""Emission posteriors without a GPU.

* cpu.align_posteriors and RecognitionLattice.align_posteriors on CPU tensors
  against the float64 reference of tests/align_post_ref.py (autograd of
  cpu._string_distance in Log with respect to the string's lexical weights):
  FrameDependent and FrameLabelDependent(1..3), FullNGram n = 0, 1, 2 and a
  random NextStateTable, ragged lengths, two batch dims; the invariants (row
  sums, total, per-frame sum, exact zeros); the collision case that the dense
  string gradient cannot separate; peaked weights against `align`; unreachable
  and invalid utterances.
* include/lt_posterior.h, the exports and lt_table_align_posteriors' host
  validation: error codes come back before any device work.
"""
import ctypes
import os
import re
import zlib

import numpy as np
import pytest
import torch

import last_torch_amd as lt
from last_torch_amd import _native
from last_torch_amd import cpu
from align_post_ref import reference
from abi_graph import dummy_graph

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include',
                      'lt_lattice.h')


def _alignment(K):
  return lt.alignments.FrameDependent() if K == 0 else lt.alignments.FrameLabelDependent(K)


def _lattice(context, K, table):
  return lt.RecognitionLattice(
      context=context, alignment=_alignment(K),
      weight_fn_cacher_factory=lambda _: lt.weight_fns.NullCacher(),
      weight_fn_factory=lambda _: lt.weight_fns.TableWeightFn(table))


def _frames(batch, T):
  return torch.arange(T, dtype=torch.float32)[:, None].expand(*batch, T, 1)


def _context(rng, V, n, C):
  if n is not None:
    return lt.contexts.FullNGram(vocab_size=V, context_size=n)
  return lt.contexts.NextStateTable(torch.tensor(rng.integers(0, C, (C, V)).astype(np.int32)))


CASES = [
    # name, V, n (FullNGram) or None (random table of C states), C, K, T, U, epsilon labels
    ('unigram_fd', 5, 0, None, 0, 12, 6, False),
    ('bigram_fd', 4, 1, None, 0, 14, 7, False),
    ('trigram_fd_eps', 3, 2, None, 0, 13, 6, True),
    ('table_fd', 6, None, 11, 0, 12, 7, True),
    ('bigram_fld1', 4, 1, None, 1, 10, 7, False),
    ('bigram_fld2', 4, 1, None, 2, 8, 9, True),
    ('table_fld3', 5, None, 7, 3, 6, 10, False),
]


def _problem(case):
  name, V, n, C, K, T, U, eps = case
  rng = np.random.default_rng(zlib.crc32(name.encode()))
  ctx = _context(rng, V, n, C)
  B = 5
  W = torch.tensor(rng.standard_normal((B, T, ctx.shape()[0], V + 1)).astype(np.float32))
  per = max(K, 1)
  # full; ragged; ragged with few labels; empty; too many labels for the frames
  nf = torch.tensor([T, T - 3, T // 2, 0, 2])
  nl = torch.tensor([min(U, T * per), min(U, (T - 3) * per) - 1, 1, 0, min(U, 2 * per + 1)])
  assert nl[4] > nf[4] * per
  lab = torch.tensor(rng.integers(0 if eps else 1, V + 1, (B, U)))
  return ctx, K, W, nf, lab, nl


def _assert_invariants(em, lp, nf, nl, K):
  """Row sums 1 below nl, total nl, per-frame sum <= 1 on FrameDependent,
  exact zeros past nl and nf, all-zero unaligned utterances; never NaN."""
  em, lp = em.double(), lp.double()
  assert torch.isfinite(em).all() and not torch.isnan(lp).any()
  B, T, U = em.shape
  tol = 1e-5 * max(T, 1)
  for b in range(B):
    n, f = int(nl[b]), int(nf[b])
    if not torch.isfinite(lp[b]):
      assert lp[b] == -torch.inf and (em[b] == 0).all()
      continue
    assert (em[b, f:] == 0).all() and (em[b, :, n:] == 0).all()
    np.testing.assert_allclose(em[b, :, :n].sum(0).numpy(), np.ones(n), atol=tol, rtol=0)
    assert abs(float(em[b].sum()) - n) <= tol * max(n, 1)
    if K == 0:
      assert (em[b].sum(-1) <= 1 + tol).all()


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_cpu_align_posteriors_match_reference(case):
  ctx, K, W, nf, lab, nl = _problem(case)
  ref_e, ref_l = reference(W, nf, lab, nl, ctx, K)
  assert torch.isfinite(ref_l[:4]).all() and ref_l[4] == -torch.inf
  _assert_invariants(ref_e, ref_l, nf, nl, K)
  B, T = W.shape[:2]
  got_e, got_l = cpu.align_posteriors(W, nf, lab, nl, ctx, _alignment(K))
  lat_e, lat_l = _lattice(ctx, K, W).align_posteriors(_frames((B,), T), nf, lab, nl)
  for e, l in ((got_e, got_l), (lat_e, lat_l)):
    assert e.dtype == torch.float32 and l.dtype == torch.float32
    assert tuple(e.shape) == (B, T, lab.shape[-1]) and tuple(l.shape) == (B,)
    assert not e.requires_grad and not l.requires_grad
    np.testing.assert_allclose(e.numpy(), ref_e.numpy(), atol=2e-5, rtol=0)
    np.testing.assert_allclose(l[:4].numpy(), ref_l[:4].numpy(), atol=1e-4, rtol=0)
    _assert_invariants(e, l, nf, nl, K)
  # float64 weights run in float64: the restatement itself, to rounding
  e64, l64 = cpu.align_posteriors(W.double(), nf, lab, nl, ctx, _alignment(K))
  assert e64.dtype == torch.float64
  np.testing.assert_allclose(e64.numpy(), ref_e.numpy(), atol=1e-13, rtol=0)
  np.testing.assert_allclose(l64[:4].numpy(), ref_l[:4].numpy(), atol=1e-12, rtol=0)


def test_two_batch_dims_and_shape_checks():
  V, T, U = 4, 9, 5
  rng = np.random.default_rng(11)
  ctx = lt.contexts.FullNGram(vocab_size=V, context_size=1)
  W = torch.tensor(rng.standard_normal((2, 3, T, ctx.num_states(), V + 1)).astype(np.float32))
  nf = torch.tensor([[9, 5, 0], [2, 9, 7]])
  nl = torch.tensor([[5, 3, 0], [4, 0, 5]])
  lab = torch.tensor(rng.integers(1, V + 1, (2, 3, U)))
  lat = _lattice(ctx, 0, W)
  em, lp = lat.align_posteriors(_frames((2, 3), T), nf, lab, nl)
  assert tuple(em.shape) == (2, 3, T, U) and tuple(lp.shape) == (2, 3)
  ref_e, ref_l = reference(W.reshape(6, *W.shape[2:]), nf.reshape(6), lab.reshape(6, U),
                           nl.reshape(6), ctx)
  np.testing.assert_allclose(em.reshape(6, T, U).numpy(), ref_e.numpy(), atol=2e-5, rtol=0)
  assert lp[1, 0] == -torch.inf and (em[1, 0] == 0).all()  # 4 labels, 2 frames
  assert lp[0, 2] == 0 and (em[0, 2] == 0).all()            # no frames, no labels
  fin = torch.isfinite(ref_l)
  np.testing.assert_allclose(lp.reshape(6)[fin].numpy(), ref_l[fin].numpy(), atol=1e-4, rtol=0)
  # log_prob is _string_forward's Log distance
  num = lat._string_forward(None, _frames((2, 3), T), nf, lab, nl, lt.semirings.Log)
  np.testing.assert_allclose(lp.reshape(6)[fin].numpy(), num.reshape(6)[fin].detach().numpy(),
                             atol=1e-4, rtol=0)
  # the expected emission frame lies inside the utterance
  when = (torch.arange(T)[:, None] * em).sum(-2)
  assert (when[0, 0] >= 0).all() and (when[0, 0] <= 8).all() and (when[0, 0].diff() > 0).all()
  with pytest.raises(ValueError):
    lat.align_posteriors(_frames((2, 3), T), nf, lab[0], nl)
  with pytest.raises(ValueError):
    lat.align_posteriors(_frames((2, 3), T), nf, lab, nl[0])


def test_collision_positions_that_the_dense_string_gradient_merges():
  """Bigram V=4, labels 1 2 1 2 1: positions 1 and 3 are both 'state 1, label
  2', positions 2 and 4 both 'state 2, label 1'. The dense Log string gradient
  (autograd of _string_forward) holds only their sums; emission separates
  them."""
  V, T, U = 4, 11, 5
  rng = np.random.default_rng(5)
  ctx = lt.contexts.FullNGram(vocab_size=V, context_size=1)
  table = torch.tensor(rng.standard_normal((1, T, ctx.num_states(), V + 1)).astype(np.float32),
                       requires_grad=True)
  lat = _lattice(ctx, 0, table)
  frames, nf, nl = _frames((1,), T), torch.tensor([T]), torch.tensor([U])
  lab = torch.tensor([[1, 2, 1, 2, 1]])
  lat._string_forward(None, frames, nf, lab, nl, lt.semirings.Log).sum().backward()
  dense = table.grad[0]                                   # [T, C, V+1]
  em, _ = lat.align_posteriors(frames, nf, lab, nl)
  em = em[0]                                              # [T, U]
  states = ctx.walk_states(lab)[0]                        # [U+1]
  assert states[1] == states[3] and states[2] == states[4]
  cells = {}
  for u in range(U):
    cells.setdefault((int(states[u]), int(lab[0, u])), []).append(u)
  assert sorted(len(us) for us in cells.values()) == [1, 2, 2]
  for (c, y), us in cells.items():
    np.testing.assert_allclose(em[:, us].sum(-1).numpy(), dense[:, c, y].numpy(), atol=5e-6,
                               rtol=0)
    if len(us) == 2:  # the two positions emit at different times
      assert float((em[:, us[0]] - em[:, us[1]]).abs().max()) > 0.1
  # every other lexical cell of the dense gradient is empty
  mask = torch.ones_like(dense, dtype=torch.bool)
  mask[..., 0] = False
  for (c, y) in cells:
    mask[:, c, y] = False
  assert (dense[mask] == 0).all()


@pytest.mark.parametrize('K', [0, 2])
def test_peaked_weights_give_aligns_one_hot(K):
  """One path ahead of every other by >= 40 nats: emission is one-hot at
  align's label_frames."""
  V, T, U, B = 4, 12, 6, 3
  rng = np.random.default_rng(21 + K)
  ctx = lt.contexts.FullNGram(vocab_size=V, context_size=1)
  # no label twice in a row: neighbouring positions then share no arc of the
  # table, so no second path runs over the raised arcs alone
  steps = rng.integers(1, V, (B, U))
  steps[:, 0] = rng.integers(0, V, B)
  lab = torch.tensor(np.cumsum(steps, axis=1) % V + 1)
  nf = torch.tensor([T, T - 2, 7])
  nl = torch.tensor([U, U - 1, 4])
  # a chosen path: label u of utterance b on frame when[b][u] (K >= 1 lets two share one)
  when = [sorted(rng.choice(int(nf[b]), int(nl[b]), replace=False).tolist()) for b in range(B)]
  if K:
    when[0][1] = when[0][0]
  states = ctx.walk_states(lab)
  W = torch.full((B, T, ctx.num_states(), V + 1), -50.0)
  W += torch.tensor(rng.uniform(-1, 1, W.shape).astype(np.float32))
  for b in range(B):
    u = 0
    for t in range(int(nf[b])):
      emitted = False
      while u < int(nl[b]) and when[b][u] == t:
        W[b, t, states[b, u], lab[b, u]] += 50.0
        u, emitted = u + 1, True
      if K or not emitted:  # a FrameLabelDependent frame ends with a blank
        W[b, t, states[b, u], 0] += 50.0
  lat = _lattice(ctx, K, W)
  frames = _frames((B,), T)
  _, label_frames, _ = lat.align(frames, nf, lab, nl)
  em, lp = lat.align_posteriors(frames, nf, lab, nl)
  assert torch.isfinite(lp).all()
  for b in range(B):
    n = int(nl[b])
    assert label_frames[b, :n].tolist() == when[b]
    onehot = torch.zeros(T, U)
    onehot[label_frames[b, :n], torch.arange(n)] = 1
    np.testing.assert_allclose(em[b].numpy(), onehot.numpy(), atol=1e-6, rtol=0)


def test_unreachable_and_invalid_utterances():
  V, T, U = 3, 8, 5
  rng = np.random.default_rng(9)
  ctx = lt.contexts.FullNGram(vocab_size=V, context_size=1)
  W = torch.tensor(rng.standard_normal((6, T, ctx.num_states(), V + 1)).astype(np.float32))
  lab = torch.tensor(rng.integers(1, V + 1, (6, U)))
  # 0: nf < nl; 1: nl > U; 2: nl < 0; 3: a -inf arc on every path; 4: -inf arcs
  # off the string's states and on one frame's lexical arcs only; 5: aligned
  nf = torch.tensor([2, T, T, T, T, T])
  nl = torch.tensor([5, U + 1, -1, 4, 4, 5])
  W[3, 2] = -torch.inf
  states = ctx.walk_states(lab)
  W[4, 5, :, 1:] = -torch.inf
  other = [c for c in range(ctx.num_states()) if c not in states[4].tolist()]
  W[4][:, other] = -torch.inf
  for K in (0, 2):
    em, lp = cpu.align_posteriors(W, nf, lab, nl, ctx, _alignment(K))
    assert not torch.isnan(em).any() and not torch.isnan(lp).any()
    assert (lp[:4] == -torch.inf).all() and (em[:4] == 0).all()
    assert torch.isfinite(lp[4:]).all()
    assert (em[4, 5] == 0).all()
    _assert_invariants(em, lp, nf, nl, K)
    ref_e, ref_l = reference(W, nf, lab, nl, ctx, K)
    np.testing.assert_allclose(em.numpy(), ref_e.numpy(), atol=2e-5, rtol=0)
    lat_e, lat_l = _lattice(ctx, K, W).align_posteriors(_frames((6,), T), nf, lab, nl)
    assert torch.equal(lat_e, em) and torch.equal(lat_l, lp)


def _define(name):
  return int(re.search(rf'#define\s+{name}\s+\(?(-?\d+)\)?', open(HEADER).read()).group(1))


def test_library_exports_what_lt_posterior_h_declares():
  """include/lt_posterior.h declares the two entry points, the library exports
  them, the binding lists them, and lt_lattice.h pulls the header in."""
  src = re.sub(r'/\*.*?\*/', '',
               open(os.path.join(os.path.dirname(HEADER), 'lt_posterior.h')).read(), flags=re.S)
  declared = sorted(set(re.findall(r'\b(lt_[a-z_]+)\s*\(', src)))
  assert declared == sorted(_native.EXPORTED_POSTERIOR) and len(declared) == 2
  for name in declared:
    assert hasattr(_native.lib(), name) and name in _native._SIG
    assert name not in _native.EXPORTED
  assert '#include "lt_posterior.h"' in open(HEADER).read()


def test_align_posteriors_host_validation_error_codes():
  lib = _native.lib()
  EINVAL, EUNSUPPORTED = _define('LT_EINVAL'), _define('LT_EUNSUPPORTED')
  null = ctypes.c_void_p(0)
  # host arrays stand in for the device pointers: nothing below dereferences them
  buf = (ctypes.c_int64 * 64)()
  p = ctypes.c_void_p(ctypes.addressof(buf))

  def graph(**kw):
    return dummy_graph(p, **kw)

  def call(g, pb, W=p, nf=p, lab=p, nl=p, em=p, lp=p, ws=null, nbytes=0):
    return lib.lt_table_align_posteriors(ctypes.byref(g), ctypes.byref(pb), W, nf, lab, nl, em, lp,
                                         ws, nbytes, null)

  def query(g, pb, nbytes):
    return lib.lt_table_align_posteriors_workspace_bytes(ctypes.byref(g), ctypes.byref(pb),
                                                         ctypes.byref(nbytes))

  TP = _native.TableProblem
  ok = TP(batch=2, max_frames=4, max_labels=3, weight_dtype=0)
  assert lib.lt_table_align_posteriors(None, ctypes.byref(ok), p, p, p, p, p, p, null, 0,
                                       null) == EINVAL
  assert call(graph(), ok, W=null) == EINVAL
  assert b'null pointer' in lib.lt_last_error()
  assert call(graph(), ok, em=null) == EINVAL
  assert b'null pointer' in lib.lt_last_error()
  assert call(graph(), ok, lp=null) == EINVAL
  assert b'null pointer' in lib.lt_last_error()
  assert call(graph(), ok, em=ctypes.c_void_p(p.value + 2)) == EINVAL
  assert b'misaligned' in lib.lt_last_error()
  assert call(graph(), TP(batch=-1, max_frames=4, max_labels=3, weight_dtype=0)) == EINVAL
  assert call(graph(), TP(batch=2, max_frames=4, max_labels=3, weight_dtype=5)) == EINVAL
  nbytes = ctypes.c_size_t(7)
  long_u = TP(batch=2, max_frames=4, max_labels=256, weight_dtype=0)
  assert call(graph(), long_u) == EUNSUPPORTED
  assert query(graph(), long_u, nbytes) == EUNSUPPORTED
  for K in (1, 2):
    assert call(graph(K=K), ok) == EUNSUPPORTED
    assert query(graph(K=K), ok, nbytes) == EUNSUPPORTED
  assert nbytes.value == 7  # a refused query writes nothing
  assert call(graph(), TP(batch=0, max_frames=4, max_labels=255, weight_dtype=0), W=null,
              em=null, lp=null) == 0
  # the history stays in LDS while max_frames rows of 8 * 64P bytes fit
  # 160 KiB beside 28 * 64P bytes of prologue arrays: P = 4 (U = 130) holds
  # 76 frames, the 77th goes to the workspace
  fits = TP(batch=3, max_frames=76, max_labels=130, weight_dtype=0)
  assert query(graph(), fits, nbytes) == 0 and nbytes.value == 0
  deep = TP(batch=3, max_frames=77, max_labels=130, weight_dtype=0)
  assert query(graph(), deep, nbytes) == 0
  assert nbytes.value >= 3 * 77 * 256 * 8
  assert call(graph(), deep, ws=null) == EINVAL
  assert b'workspace' in lib.lt_last_error()
  bench = TP(batch=64, max_frames=1000, max_labels=100, weight_dtype=1)
  assert query(graph(), bench, nbytes) == 0 and nbytes.value >= 64 * 1000 * 128 * 8
