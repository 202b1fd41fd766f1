"""Emission posteriors on the GPU (RecognitionLattice.align_posteriors ->
lt_table_align_posteriors, lt_align_post.hip) against the float64 reference of
tests/align_post_ref.py (autograd of cpu._string_distance in Log), at the
kernel's lane and slice boundaries (U = 63 .. 255), its ring and midpoint
boundaries, a trigram with epsilons, random next-state tables (one too large
to stage in LDS), bf16 weights, -inf arcs, a history that does not fit LDS,
and the two shapes past the kernel's range (the on-device restatement).

Bounds. The same reference run in float32 is the yardstick: its max abs error
against the float64 run, on the same inputs, computed here at run time. The
kernel's error on emission and on log_prob may be at most 4x the yardstick's
(a different summation order and the hardware exp / log). A column of
emission sums T terms, so its sum may miss 1 by that bound x T. log_prob and
_string_forward(..., Log) are two fp32 evaluations each within 4x of the
truth, so they may differ by 8x the yardstick's log_prob error. Every figure
is printed before it is asserted (pytest -s shows them).

DESIGN.md section 3k lists the measured figures of every case: no case needs
more than 2.7x on emission (bf16 at U = 130), 1.0x on log_prob.
"""
import zlib

import numpy as np
import pytest
import torch

import last_torch_amd as lt
from last_torch_amd import _native as nat
from align_post_ref import reference, yardstick
import poisoned_buffers

pytestmark = pytest.mark.gpu

FACTOR = 4.0  # kernel error <= FACTOR * the float32 yardstick's error


def _lattice(context, K, table):
  align = lt.alignments.FrameDependent() if K == 0 else lt.alignments.FrameLabelDependent(K)
  return lt.RecognitionLattice(
      context=context, alignment=align,
      weight_fn_cacher_factory=lambda _: lt.weight_fns.NullCacher(),
      weight_fn_factory=lambda _: lt.weight_fns.TableWeightFn(table))


def _frames(batch, T, device):
  return torch.arange(T, dtype=torch.float32, device=device)[:, None].expand(*batch, T, 1)


def _lengths(rng, T, U, K):
  """test_gpu_align._lengths' four utterances: full length with every label
  the frames carry (num_labels = U, or T - 3 where T < U on FrameDependent);
  full length with a little less; empty; three frames with one label too
  many (unaligned)."""
  per = max(K, 1)
  nf = np.array([T, T, 0, 3], np.int32)
  full = U if T * per >= U else T * per - 3
  nl = np.array([full, max(0, min(U, T * per) - int(rng.integers(0, 4))), 0,
                 min(U, 3 * per + 1)], np.int32)
  assert nl[3] > nf[3] * per
  return nf, nl


CASES = [
    # name, V, n (FullNGram) or None (random table of C states), C, K, T, U, dtype, epsilon, -inf
    ('bigram_u63', 32, 1, None, 0, 70, 63, 'f32', False, False),
    ('bigram_u64', 32, 1, None, 0, 70, 64, 'f32', False, False),   # P 1 -> 2
    ('bigram_u65', 32, 1, None, 0, 70, 65, 'f32', False, False),
    ('bigram_u127', 32, 1, None, 0, 70, 127, 'f32', False, False),
    ('bigram_u128', 32, 1, None, 0, 70, 128, 'f32', False, False),  # P 2 -> 4
    ('bigram_u127_t130', 32, 1, None, 0, 130, 127, 'f32', False, False),  # every lane of P = 2 live
    ('bigram_u255_t260', 32, 1, None, 0, 260, 255, 'f32', False, False),
    ('trigram_v5_eps', 5, 2, None, 0, 30, 9, 'f32', True, False),
    ('table_c17_v6', 6, None, 17, 0, 30, 9, 'f32', True, False),
    ('table_c300_v28', 28, None, 300, 0, 20, 9, 'f32', True, False),  # too large to stage in LDS
    ('bigram_bf16_u65', 32, 1, None, 0, 70, 65, 'bf16', False, False),
    ('bigram_v4_minus_inf', 4, 1, None, 0, 30, 9, 'f32', False, True),
    # history rows of 8 * 256 bytes beside 28 * 256 bytes of prologue arrays:
    # 76 frames fit 160 KiB of LDS, the 77th sends the history to the workspace
    ('bigram_u130_t76_lds', 8, 1, None, 0, 76, 130, 'f32', False, False),
    ('bigram_u130_t77_ws', 8, 1, None, 0, 77, 130, 'f32', False, False),
    ('bigram_bf16_u130_t77_ws', 8, 1, None, 0, 77, 130, 'bf16', False, False),
]
_BY_NAME = {c[0]: c for c in CASES}
_PROBLEMS = {}


def _table(rng, V, n, C):
  if n is not None:
    ctx = lt.contexts.FullNGram(vocab_size=V, context_size=n)
  else:
    ctx = lt.contexts.NextStateTable(torch.tensor(rng.integers(0, C, (C, V)).astype(np.int32)))
  return ctx


def _problem(name, variant=''):
  """(context, K, W, nf, labels, nl, dtype, emission error of the yardstick,
  its log_prob error, float64 emission, float64 log_prob) of a case, computed
  once and shared by the tests that use it (nothing changes them)."""
  key = name + variant
  if key in _PROBLEMS:
    return _PROBLEMS[key]
  _, V, n, C, K, T, U, dt, eps, minf = _BY_NAME[name]
  rng = np.random.default_rng(zlib.crc32(key.encode()))
  ctx = _table(rng, V, n, C)
  B = 4
  W = rng.standard_normal((B, T, ctx.shape()[0], V + 1)).astype(np.float32)
  if minf:
    W[rng.random(W.shape) < 0.05] = -np.inf
  W = torch.tensor(W)
  if dt == 'bf16':
    W = W.bfloat16().float()
  nf, nl = _lengths(rng, T, U, K)
  lab = rng.integers(0 if eps else 1, V + 1, (B, U)).astype(np.int32)
  nf, nl, lab = torch.tensor(nf), torch.tensor(nl), torch.tensor(lab)
  e_err, l_err, e64, l64 = yardstick(W, nf, lab, nl, ctx, K)
  # the reference alone leaves at most the short utterance unaligned
  assert torch.isfinite(l64[:3]).all() and l64[3] == -torch.inf and l64[2] == 0
  _PROBLEMS[key] = (ctx, K, W, nf, lab, nl, dt, e_err, l_err, e64, l64)
  return _PROBLEMS[key]


def _run(ctx, K, W, nf, lab, nl, dt, device):
  """(emission, log_prob, _string_forward's Log distance) on the device."""
  B, T = W.shape[:2]
  Wd = W.to(device)
  lat = _lattice(ctx, K, Wd)
  nfd, labd, nld = nf.to(device), lab.to(device), nl.to(device)
  if dt == 'bf16':
    # TableWeightFn hands out fp32: the bf16 kernel through the binding
    graph = lat._graph(device)
    em, lp = nat.table_align_posteriors(graph, Wd.bfloat16().contiguous(), nfd, labd, nld)
    sf = nat.table_num_forward(graph, Wd.bfloat16().contiguous(), nfd, labd, nld,
                               nat.SEMIRING_LOG)
  else:
    frames = _frames((B,), T, device)
    em, lp = lat.align_posteriors(frames, nfd, labd, nld)
    sf = lat._string_forward(None, frames, nfd, labd, nld, lt.semirings.Log)
  return em, lp, sf


def _check(name, em, lp, sf, nf, nl, e_err, l_err, e64, l64):
  B, T, U = e64.shape
  assert em.dtype == torch.float32 and lp.dtype == torch.float32
  assert tuple(em.shape) == (B, T, U) and tuple(lp.shape) == (B,)
  em, lp = em.cpu(), lp.cpu()
  assert torch.isfinite(em).all() and not torch.isnan(lp).any()
  fin = torch.isfinite(l64)
  assert torch.equal(torch.isfinite(lp), fin) and (lp[~fin] == -torch.inf).all()
  k_e = float((em.double() - e64).abs().max()) if em.numel() else 0.0
  k_l = float((lp.double() - l64)[fin].abs().max())
  cols = [em[b, :, :int(nl[b])].double().sum(0) for b in range(B) if fin[b]]
  k_s = max([float((c - 1).abs().max()) for c in cols if c.numel()] or [0.0])
  print(f'\n{name}: emission kernel {k_e:.3g} yardstick {e_err:.3g} | log_prob kernel {k_l:.3g} '
        f'yardstick {l_err:.3g} | column sums off 1 by {k_s:.3g} (T = {T})', end='')
  if sf is not None:
    k_f = float((lp.double() - sf.cpu().double())[fin].abs().max())
    print(f' | log_prob vs _string_forward {k_f:.3g}', end='')
  # exact zeros past num_labels and num_frames; unaligned utterances all zero
  for b in range(B):
    assert (em[b, int(nf[b]):] == 0).all() and (em[b, :, max(int(nl[b]), 0):] == 0).all()
    if not fin[b]:
      assert (em[b] == 0).all()
  assert k_e <= FACTOR * e_err, (k_e, e_err)
  assert k_l <= FACTOR * l_err, (k_l, l_err)
  assert k_s <= FACTOR * e_err * T, (k_s, e_err, T)
  if sf is not None:
    assert k_f <= 2 * FACTOR * l_err, (k_f, l_err)


@pytest.mark.parametrize('name', [c[0] for c in CASES])
def test_align_posteriors_match_reference(cuda, name):
  ctx, K, W, nf, lab, nl, dt, e_err, l_err, e64, l64 = _problem(name)
  graph = _lattice(ctx, K, W.to(cuda))._graph(cuda)
  assert nat.table_align_posteriors_supported(graph, W.to(cuda), lab.to(cuda))
  em, lp, sf = _run(ctx, K, W, nf, lab, nl, dt, cuda)
  _check(name, em, lp, sf, nf, nl, e_err, l_err, e64, l64)


def test_ring_and_midpoint_boundaries(cuda):
  """num_frames 1, 2, 3, 15, 16, 17, 33 in one batch at U = 9: odd and even
  midpoints, phases shorter than, equal to and one past the 16-frame ring."""
  V, T, U = 6, 33, 9
  rng = np.random.default_rng(33)
  ctx = lt.contexts.FullNGram(vocab_size=V, context_size=1)
  W = torch.tensor(rng.standard_normal((7, T, ctx.num_states(), V + 1)).astype(np.float32))
  nf = torch.tensor([1, 2, 3, 15, 16, 17, 33], dtype=torch.int32)
  nl = torch.tensor([1, 2, 2, 9, 9, 8, 9], dtype=torch.int32)
  lab = torch.tensor(rng.integers(1, V + 1, (7, U)).astype(np.int32))
  e_err, l_err, e64, l64 = yardstick(W, nf, lab, nl, ctx)
  assert torch.isfinite(l64).all()
  em, lp, sf = _run(ctx, 0, W, nf, lab, nl, 'f32', cuda)
  _check('ring_midpoint', em, lp, sf, nf, nl, e_err, l_err, e64, l64)


@pytest.mark.parametrize('name,K,V,T,U', [('fld2_u12', 2, 4, 20, 12), ('fd_u256', 0, 8, 260, 256)])
def test_beyond_kernel_range_runs_the_restatement_on_the_device(cuda, name, K, V, T, U):
  """FrameLabelDependent(2) and U = 256 are past the kernel: the binding
  refuses (LT_EUNSUPPORTED) and RecognitionLattice.align_posteriors answers
  with the torch restatement on the tensors' own device."""
  rng = np.random.default_rng(zlib.crc32(name.encode()))
  ctx = lt.contexts.FullNGram(vocab_size=V, context_size=1)
  W = torch.tensor(rng.standard_normal((4, T, ctx.num_states(), V + 1)).astype(np.float32))
  nf, nl = _lengths(rng, T, U, K)
  nf, nl = torch.tensor(nf), torch.tensor(nl)
  lab = torch.tensor(rng.integers(1, V + 1, (4, U)).astype(np.int32))
  e_err, l_err, e64, l64 = yardstick(W, nf, lab, nl, ctx, K)
  assert torch.isfinite(l64[:3]).all() and l64[3] == -torch.inf
  lat = _lattice(ctx, K, W.to(cuda))
  args = (lat._graph(cuda), W.to(cuda), nf.to(cuda), lab.to(cuda), nl.to(cuda))
  assert not nat.table_align_posteriors_supported(args[0], args[1], args[3])
  with pytest.raises(nat.LatticeLibraryError, match=r'\(-2\)'):
    nat.table_align_posteriors(*args)
  em, lp = lat.align_posteriors(_frames((4,), T, cuda), nf.to(cuda), lab.to(cuda), nl.to(cuda))
  assert em.device.type == 'cuda' and lp.device.type == 'cuda'
  _check(name, em, lp, None, nf, nl, e_err, l_err, e64, l64)


def test_batch_dims_on_the_device(cuda):
  V, T, U = 5, 25, 7
  rng = np.random.default_rng(3)
  ctx = lt.contexts.FullNGram(vocab_size=V, context_size=1)
  W = torch.tensor(rng.standard_normal((2, 3, T, ctx.num_states(), V + 1)).astype(np.float32))
  nf = torch.tensor([[25, 10, 0], [3, 25, 17]])
  nl = torch.tensor([[7, 3, 0], [5, 0, 7]])
  lab = torch.tensor(rng.integers(1, V + 1, (2, 3, U)))
  lat = _lattice(ctx, 0, W.to(cuda))
  frames = _frames((2, 3), T, cuda)
  em, lp = lat.align_posteriors(frames, nf.to(cuda), lab.to(cuda), nl.to(cuda))
  assert tuple(em.shape) == (2, 3, T, U) and tuple(lp.shape) == (2, 3)
  assert em.device == frames.device and not em.requires_grad
  e_err, l_err, e64, l64 = yardstick(W.reshape(6, *W.shape[2:]), nf.reshape(6),
                                     lab.reshape(6, U), nl.reshape(6), ctx)
  _check('batch_dims', em.reshape(6, T, U), lp.reshape(6), None, nf.reshape(6), nl.reshape(6),
         e_err, l_err, e64, l64)
  assert lp[1, 0] == -torch.inf and lp[0, 2] == 0
  with pytest.raises(ValueError):
    lat.align_posteriors(frames, nf.to(cuda), lab[0].to(cuda), nl.to(cuda))


@pytest.mark.parametrize('name', ['bigram_u130_t76_lds', 'bigram_u130_t77_ws'])
def test_poisoned_and_stale_buffers_and_determinism(cuda, name):
  """Every output and workspace byte is the call's own: the results on 0xFF
  memory, and on the memory a finished call on another problem of the same
  shape left behind, are bit-equal to a plain run; so are two plain runs."""
  ctx, K, W, nf, lab, nl, dt, *_ = _problem(name)
  ctx2, _, W2, nf2, lab2, nl2, *_ = _problem(name, '-other')
  lat = _lattice(ctx, K, W.to(cuda))
  graph = lat._graph(cuda)

  def call(W_, nf_, lab_, nl_):
    return nat.table_align_posteriors(graph, W_.to(cuda), nf_.to(cuda), lab_.to(cuda),
                                      nl_.to(cuda))

  nbytes = nat.ctypes.c_size_t(0)
  pb = nat._tproblem(graph, W.to(cuda), lab.shape[-1])
  nat._check(nat.lib().lt_table_align_posteriors_workspace_bytes(
      nat.ctypes.byref(graph.g), nat.ctypes.byref(pb), nat.ctypes.byref(nbytes)), 'query')
  assert (nbytes.value > 0) == name.endswith('_ws')
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
