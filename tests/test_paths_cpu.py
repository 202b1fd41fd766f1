"""Path scoring, edit distance and sampled risk without a GPU
(RecognitionLattice.path_weights / sampled_risk and last_torch_amd.edit_distance
on CPU tensors -> cpu.path_weights / cpu.edit_distance, the definitions of
include/lt_paths.h in torch ops), against the NumPy restatement path_ref.

* cpu.path_weights: weights bit-equal to the fp32 reverse-order sum, states
  exact, on three lattices with ragged / one-frame / empty utterances; the
  labels `sample` returned score to its path_weights bit for bit; `align`'s
  within the fp32 bound of a T-term sum, T 2^-24 sum |w|; autograd equals the
  float64 scatter; an invalid label gives -inf and a zero gradient.
* cpu.edit_distance: exact against a two-row Levenshtein, and the edge cases
  of the definition.
* The C ABI's host validation of the three entry points.
* The estimator: on the 81-path bigram of test_sample_cpu (V = 2, T = 4) with
  a fixed random cost per label sequence, R, Cov(c, 1[a]) and
  mu22_a = E[(c - R)^2 (1[a] - m_a)^2] are enumerated in float64; one
  sampled_risk call at S = 4096 must give |risk - R| <= 6 sigma_c / sqrt(S)
  and, for every arc, |dW_a - Cov_a| <= 6 sqrt(mu22_a / S) + 1e-6: six
  standard deviations of a sample mean / a sample covariance.
"""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import last_torch_amd as lt
from last_torch_amd import _native
from last_torch_amd import cpu
import path_ref
import sample_ref
from abi_graph import dummy_graph

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include')

CONTEXTS = {
    'bigram_v32': lambda rng: lt.contexts.FullNGram(vocab_size=32, context_size=1),
    'trigram_v5': lambda rng: lt.contexts.FullNGram(vocab_size=5, context_size=2),
    'table_c17_v6': lambda rng: lt.contexts.NextStateTable(sample_ref.random_table(rng, 17, 6)),
}


def _lattice(context, table, K=0):
  align = lt.alignments.FrameDependent() if K == 0 else lt.alignments.FrameLabelDependent(K)
  return lt.RecognitionLattice(
      context=context, alignment=align,
      weight_fn_cacher_factory=lambda _: lt.weight_fns.NullCacher(),
      weight_fn_factory=lambda _: lt.weight_fns.TableWeightFn(table))


def _frames(B, T):
  return torch.arange(T, dtype=torch.float32)[None, :, None].expand(B, T, 1)


def _problem(name, T=11, S=3, seed=0):
  rng = np.random.default_rng(sum(map(ord, name)) + seed)
  context = CONTEXTS[name](rng)
  table = sample_ref.table_of(context)
  C, V = table.shape
  nf = [T, T - 3, 1, 0]
  B = len(nf)
  W = rng.standard_normal([B, T, C, V + 1]).astype(np.float32)
  labels = rng.integers(0, V + 1, [B, S, T])
  labels[rng.random([B, S, T]) < 0.4] = 0
  return context, table, W, nf, labels


@pytest.mark.parametrize('name', list(CONTEXTS))
def test_path_weights_against_the_reference(name):
  context, table, W, nf, labels = _problem(name)
  got, states = cpu.path_weights(torch.tensor(W), torch.tensor(nf), torch.tensor(labels), context)
  w32, w64, mag, want_states = path_ref.score(W, nf, table, labels)
  assert got.dtype == torch.float32 and states.dtype == torch.int32
  np.testing.assert_array_equal(got.numpy(), w32)          # the same fp32 adds, the same order
  np.testing.assert_array_equal(states.numpy(), want_states)
  assert (np.abs(w32 - w64) <= W.shape[1] * 2.0**-24 * mag).all()
  assert not got[3].any() and (states[3] == -1).all()      # num_frames = 0: weight 0


@pytest.mark.parametrize('name', list(CONTEXTS))
def test_method_matches_cpu_function_and_batch_dims(name):
  context, table, W, nf, labels = _problem(name)
  lat = _lattice(context, torch.tensor(W).reshape(2, 2, *W.shape[1:]))
  T = W.shape[1]
  got = lat.path_weights(_frames(4, T).reshape(2, 2, T, 1), torch.tensor(nf).reshape(2, 2),
                         torch.tensor(labels).reshape(2, 2, -1, T))
  assert tuple(got.shape) == (2, 2, labels.shape[1])
  np.testing.assert_array_equal(got.reshape(4, -1).numpy(),
                                path_ref.score(W, nf, table, labels)[0])


@pytest.mark.parametrize('name', list(CONTEXTS))
def test_sampled_labels_score_to_the_samplers_weight_bit_for_bit(name):
  context, table, W, nf, _ = _problem(name)
  B, T = W.shape[:2]
  lat = _lattice(context, torch.tensor(W))
  labels, weights, _ = lat.sample(_frames(B, T), torch.tensor(nf), 6, 41)
  got = lat.path_weights(_frames(B, T), torch.tensor(nf), labels)
  np.testing.assert_array_equal(got.numpy(), weights.numpy())
  np.testing.assert_array_equal(got.numpy(), path_ref.score(W, nf, table, labels.numpy())[0])


@pytest.mark.parametrize('name', list(CONTEXTS))
def test_aligned_labels_score_to_the_alignments_weight(name):
  context, table, W, nf, _ = _problem(name)
  rng = np.random.default_rng(2)
  B, T = W.shape[:2]
  V = table.shape[1]
  U = 4
  lab = torch.tensor(rng.integers(1, V + 1, [B, U]))
  nl = torch.tensor([4, 3, 1, 0])
  lat = _lattice(context, torch.tensor(W))
  paths, _, weights = lat.align(_frames(B, T), torch.tensor(nf), lab, nl)
  got = lat.path_weights(_frames(B, T), torch.tensor(nf), paths[:, None])
  _, _, mag, _ = path_ref.score(W, nf, table, paths[:, None].numpy())
  assert np.isfinite(weights.numpy()).all()
  err = np.abs(got[:, 0].numpy().astype(np.float64) - weights.numpy())
  assert (err <= T * 2.0**-24 * mag[:, 0]).all(), (err, mag)


@pytest.mark.parametrize('name', list(CONTEXTS))
def test_autograd_is_the_scatter(name):
  context, table, W, nf, labels = _problem(name, S=5)
  labels[:, 2] = labels[:, 0]                    # paths that share every arc
  rng = np.random.default_rng(8)
  Wt = torch.tensor(W, requires_grad=True)
  got, states = cpu.path_weights(Wt, torch.tensor(nf), torch.tensor(labels), context)
  for grad, exact in ((rng.integers(-3, 4, got.shape).astype(np.float32), True),
                      (rng.standard_normal(got.shape).astype(np.float32), False)):
    Wt.grad = None
    got.backward(torch.tensor(grad), retain_graph=True)
    want, mag = path_ref.scatter(W.shape, nf, labels, states.numpy(), grad)
    if exact:
      np.testing.assert_array_equal(Wt.grad.numpy(), want)
    else:
      assert (np.abs(Wt.grad.numpy() - want) <= labels.shape[1] * 2.0**-24 * mag).all()
    assert not Wt.grad.numpy()[want == 0].any()


def test_invalid_label_gives_minus_inf_and_no_gradient():
  context, table, W, nf, labels = _problem('table_c17_v6')
  V = table.shape[1]
  labels[0, 1, 4] = V + 1
  labels[1, 0, 2] = -1
  labels[1, 2, 9] = V + 5                         # a padding frame (nf = 8): ignored
  Wt = torch.tensor(W, requires_grad=True)
  got, states = cpu.path_weights(Wt, torch.tensor(nf), torch.tensor(labels), context)
  w32, _, _, want_states = path_ref.score(W, nf, table, labels)
  np.testing.assert_array_equal(got.detach().numpy(), w32)
  np.testing.assert_array_equal(states.numpy(), want_states)
  assert got[0, 1] == -np.inf and got[1, 0] == -np.inf and np.isfinite(got[1, 2].item())
  assert (states[0, 1] == -1).all() and (states[1, 0] == -1).all()
  assert not torch.isnan(got).any()
  grad = np.ones(got.shape, np.float32)
  got.backward(torch.tensor(grad))
  want, _ = path_ref.scatter(W.shape, nf, labels, want_states, grad)
  np.testing.assert_array_equal(Wt.grad.numpy(), want)


def test_frame_label_dependent_raises():
  context = lt.contexts.FullNGram(vocab_size=3, context_size=1)
  lat = _lattice(context, torch.zeros([1, 4, 4, 4]), K=2)
  with pytest.raises(NotImplementedError):
    lat.path_weights(torch.zeros([1, 4, 1]), torch.tensor([4]), torch.zeros([1, 2, 4]).long())
  with pytest.raises(NotImplementedError):
    lat.sampled_risk(torch.zeros([1, 4, 1]), torch.tensor([4]), torch.ones([1, 2]).long(),
                     torch.tensor([2]), 2, 0)


# ---------------------------------------------------------------------------
# edit distance
# ---------------------------------------------------------------------------
def _ed(hyp, nf, ref, nl):
  got = cpu.edit_distance(torch.tensor(hyp), None if nf is None else torch.tensor(nf),
                          torch.tensor(ref), torch.tensor(nl))
  want = path_ref.edit_distance(hyp, nf, ref, nl)
  assert got[0].dtype == torch.int32 and got[1].dtype == torch.int32
  np.testing.assert_array_equal(got[0].numpy(), want[0])
  np.testing.assert_array_equal(got[1].numpy(), want[1])
  pub = lt.edit_distance(torch.tensor(hyp), None if nf is None else torch.tensor(nf),
                         torch.tensor(ref), torch.tensor(nl))
  np.testing.assert_array_equal(pub.numpy(), want[0])
  return want[0]


@pytest.mark.parametrize('U,T', [(0, 5), (1, 1), (7, 12), (12, 7), (30, 30)])
def test_edit_distance_against_the_reference(U, T):
  rng = np.random.default_rng(100 * U + T)
  B, S = 4, 3
  hyp = rng.integers(0, 4, [B, S, T])             # a 3-symbol alphabet plus blanks
  ref = rng.integers(0, 4, [B, U]).astype(np.int32)
  nf = [T, max(T - 3, 0), 1, 0]
  nl = [U, max(U - 2, 0), min(U, 1), 0]
  _ed(hyp, nf, ref, nl)
  _ed(hyp, None, ref, nl)


def test_edit_distance_edge_cases():
  ref = np.array([[1, 2, 0, 3, 2], [1, 2, 0, 3, 2], [0, 0, 0, 0, 0], [3, 3, 3, 3, 3]], np.int32)
  hyp = np.zeros([4, 3, 9], np.int64)
  hyp[:, 0, [1, 4, 6, 8]] = [1, 2, 3, 2]          # the tokens of ref rows 0 / 1, blanks between
  hyp[:, 1] = 0                                   # the empty hypothesis
  hyp[:, 2, :5] = [2, 2, 1, 0, 7]
  d = _ed(hyp, [9, 9, 9, 9], ref, [5, 5, 5, 5])
  assert d[0, 0] == 0 and d[1, 0] == 0            # identical (zeros in ref are skipped)
  assert d[0, 1] == 4                             # the empty hypothesis: the ref length
  assert (d[2] == [4, 0, 4]).all()                # the empty reference: the hyp length
  d = _ed(hyp, [9, 7, 9, 9], ref, [5, 5, 5, 5])
  assert d[1, 0] == 1                             # the token past num_frames is ignored
  d = _ed(hyp, [9, 9, 9, 9], ref, [5, 6, -1, 2])
  assert (d[1] == -1).all() and (d[2] == -1).all()  # num_labels out of range
  assert d[3, 1] == 2


# ---------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------
def _define(name):
  src = open(os.path.join(INCLUDE, 'lt_lattice.h')).read()
  return int(re.search(rf'#define\s+{name}\s+\(?(-?\d+)\)?', src).group(1))


def test_library_exports_what_lt_paths_h_declares():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(INCLUDE, 'lt_paths.h')).read(), flags=re.S)
  declared = sorted(set(re.findall(r'\b(lt_[a-z_]+)\s*\(', src)))
  assert declared == sorted(_native.EXPORTED_PATHS) and len(declared) == 3
  for name in declared:
    assert hasattr(_native.lib(), name) and name in _native._SIG
    assert name not in _native.EXPORTED
  assert '#include "lt_paths.h"' in open(os.path.join(INCLUDE, 'lt_lattice.h')).read()


def test_host_validation_error_codes():
  lib = _native.lib()
  EINVAL, EUNSUPPORTED = _define('LT_EINVAL'), _define('LT_EUNSUPPORTED')
  null = ctypes.c_void_p(0)
  # host arrays stand in for the device pointers: nothing below dereferences
  # them, and no call below passes validation with a batch to launch
  buf = (ctypes.c_int64 * 64)()
  p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
  TP = _native.TableProblem
  ok = TP(batch=2, max_frames=4, max_labels=0, weight_dtype=0)
  empty = TP(batch=0, max_frames=4, max_labels=0, weight_dtype=0)

  def graph(**kw):
    return dummy_graph(p, **kw)

  def score(g, pb, W=p, nf=p, lab=p, S=4, pw=p, st=p):
    return lib.lt_table_path_score(ctypes.byref(g), ctypes.byref(pb), W, nf, lab, S, pw, st, null)

  def scatter(g, pb, nf=p, lab=p, st=p, S=4, grad=p, dW=p):
    return lib.lt_table_path_scatter(ctypes.byref(g), ctypes.byref(pb), nf, lab, st, S, grad, dW,
                                     null)

  for fn in (score, scatter):
    assert fn(graph(), ok, S=0) == EINVAL
    assert b'num_paths' in lib.lt_last_error()
    assert fn(graph(), ok, nf=null) == EINVAL
    assert b'null pointer' in lib.lt_last_error()
    assert fn(graph(), ok, lab=null) == EINVAL
    assert fn(graph(K=1), ok) == EUNSUPPORTED
    assert b'FrameLabelDependent' in lib.lt_last_error()
    assert fn(graph(C=1 << 20, V=1 << 12), ok) == EUNSUPPORTED
    assert fn(graph(), TP(batch=1 << 20, max_frames=4, max_labels=0, weight_dtype=0),
              S=1 << 12) == EUNSUPPORTED
    assert fn(graph(), TP(batch=2, max_frames=4, max_labels=0, weight_dtype=5)) == EINVAL
    assert fn(graph(), empty, nf=null, lab=null) == 0
  assert lib.lt_table_path_score(None, ctypes.byref(ok), p, p, p, 4, p, p, null) == EINVAL
  assert score(graph(), ok, pw=null) == EINVAL
  assert score(graph(), ok, W=null) == EINVAL
  assert score(graph(), ok, lab=ctypes.c_void_p(p.value + 4)) == EINVAL
  assert b'misaligned' in lib.lt_last_error()
  # the LDS rows bound T
  assert score(graph(), TP(batch=0, max_frames=40960, max_labels=0, weight_dtype=0)) == 0
  assert score(graph(), TP(batch=2, max_frames=40961, max_labels=0, weight_dtype=0)) == \
      EUNSUPPORTED
  assert scatter(graph(), ok, st=null) == EINVAL
  assert scatter(graph(), ok, grad=null) == EINVAL
  assert scatter(graph(), ok, dW=null) == EINVAL

  def edit(B=2, S=3, T=4, U=5, hyp=p, nf=p, ref=p, nl=p, dist=p, length=p):
    return lib.lt_edit_distance(B, S, T, U, hyp, nf, ref, nl, dist, length, null)

  assert edit(S=0) == EINVAL
  assert b'num_hyps' in lib.lt_last_error()
  assert edit(T=-1) == EINVAL
  assert edit(hyp=null) == EINVAL
  assert edit(ref=null) == EINVAL
  assert edit(nl=null) == EINVAL
  assert edit(dist=null) == EINVAL
  assert b'null pointer' in lib.lt_last_error()
  assert edit(U=1024) == EUNSUPPORTED           # 1025 cells
  assert b'max_labels' in lib.lt_last_error()
  assert edit(B=0, U=1023) == 0
  assert edit(B=1 << 20, S=1 << 12) == EUNSUPPORTED
  assert _native.edit_distance_supported(1023) and not _native.edit_distance_supported(1024)


# ---------------------------------------------------------------------------
# the estimator
# ---------------------------------------------------------------------------
def _enumerated():
  """The 81-path bigram with a fixed random cost per label sequence."""
  rng = np.random.default_rng(7)
  context = lt.contexts.FullNGram(vocab_size=2, context_size=1)
  table = sample_ref.table_of(context)
  T = 4
  W = rng.standard_normal([1, T, 3, 3]).astype(np.float32)
  probs = sample_ref.path_probabilities(W[0], table, T)
  seqs = list(probs)
  assert len(seqs) == 81
  p = np.array([probs[s] for s in seqs])
  cost = rng.uniform(0, 3, [81])
  index = {s: i for i, s in enumerate(itertools.product(range(3), repeat=T))}
  c = np.array([cost[index[s]] for s in seqs])
  ind = np.zeros([81, T, 3, 3])
  for i, s in enumerate(seqs):
    for t, (q, y) in enumerate(zip(sample_ref.walk(s, table), s)):
      ind[i, t, q, y] = 1
  R = (p * c).sum()
  m = np.einsum('i,itqy->tqy', p, ind)
  cov = np.einsum('i,itqy->tqy', p * (c - R), ind - m)
  mu22 = np.einsum('i,itqy->tqy', p * (c - R)**2, (ind - m)**2)
  sigma = np.sqrt((p * (c - R)**2).sum())
  cost_table = torch.tensor(cost, dtype=torch.float32)

  def cost_fn(alignment_labels, num_frames):
    assert tuple(alignment_labels.shape[-1:]) == (T,) and tuple(num_frames.shape) == (1,)
    code = (alignment_labels * torch.tensor([27, 9, 3, 1])).sum(-1)
    return cost_table[code]

  return context, table, W, cost_fn, R, m, cov, mu22, sigma


def _count_den_forward(monkeypatch):
  calls = []
  real = cpu.den_forward

  def counted(*a, **k):
    calls.append(torch.is_grad_enabled())
    return real(*a, **k)

  monkeypatch.setattr(cpu, 'den_forward', counted)
  return calls


def test_estimator_meets_the_enumerated_risk_and_covariance(monkeypatch):
  context, table, W, cost_fn, R, _, cov, mu22, sigma = _enumerated()
  S = 4096
  Wt = torch.tensor(W, requires_grad=True)
  lat = _lattice(context, Wt)
  calls = _count_den_forward(monkeypatch)
  risk, costs, paths = lat.sampled_risk(_frames(1, 4), torch.tensor([4]), None, None, S, 20260102,
                                        cost_fn=cost_fn)
  assert tuple(risk.shape) == (1,) and tuple(costs.shape) == (1, S)
  assert tuple(paths.shape) == (1, S, 4) and not costs.requires_grad
  # drawn exactly as `sample` draws
  np.testing.assert_array_equal(
      paths.numpy(), lat.sample(_frames(1, 4), torch.tensor([4]), S, 20260102)[0].numpy())
  del calls[1:]
  assert risk.item() == costs.mean(-1).item()
  print(f'risk {risk.item():.5f} against R = {R:.5f}, bound {6 * sigma / np.sqrt(S):.5f}')
  assert abs(risk.item() - R) <= 6 * sigma / np.sqrt(S)
  risk.sum().backward()
  got = Wt.grad.numpy()[0].astype(np.float64)
  units = np.abs(got - cov) / (6 * np.sqrt(mu22 / S) + 1e-6)
  print(f'gradient: worst arc at {units.max():.3f} of its bound')
  assert (units <= 1).all()
  # the log Z pass ran once, outside the graph: no marginal pass in the backward
  assert calls == [False]
  # and the gradient is exactly the scatter of the advantages
  c = costs.numpy()
  adv = (c - risk.detach().numpy()[:, None]) / np.float32(S - 1)
  states = path_ref.score(W, [4], table, paths.numpy())[3]
  want, mag = path_ref.scatter(W.shape, [4], paths.numpy(), states, adv)
  assert (np.abs(Wt.grad.numpy() - want) <= S * 2.0**-24 * mag + 1e-12).all()


def test_single_sample_gradient_is_cost_times_indicator_minus_marginals(monkeypatch):
  context, table, W, cost_fn, _, m, _, _, _ = _enumerated()
  Wt = torch.tensor(W, requires_grad=True)
  lat = _lattice(context, Wt)
  calls = _count_den_forward(monkeypatch)
  risk, costs, paths = lat.sampled_risk(_frames(1, 4), torch.tensor([4]), None, None, 1, 5,
                                        cost_fn=cost_fn)
  assert calls == [True] and risk.item() == costs.item()
  risk.sum().backward()
  states = path_ref.score(W, [4], table, paths.numpy())[3]
  ind, _ = path_ref.scatter(W.shape, [4], paths.numpy(), states, np.ones([1, 1]))
  want = costs.item() * (ind[0] - m)
  np.testing.assert_allclose(Wt.grad.numpy()[0], want, rtol=1e-4, atol=1e-5)


def test_default_cost_is_the_edit_distance_and_degenerate_utterances():
  rng = np.random.default_rng(12)
  context = lt.contexts.FullNGram(vocab_size=3, context_size=1)
  B, T, S, U = 3, 8, 5, 4
  W = rng.standard_normal([B, T, 4, 4]).astype(np.float32)
  W[1] = -np.inf                                   # no path at all: unsampled
  Wt = torch.tensor(W, requires_grad=True)
  lat = _lattice(context, Wt)
  ref = rng.integers(1, 4, [B, U]).astype(np.int32)
  nl, nf = [4, 3, 2], [T, T, 5]
  risk, costs, paths = lat.sampled_risk(_frames(B, T), torch.tensor(nf), torch.tensor(ref),
                                        torch.tensor(nl), 1, 3)   # S = 1: through log Z
  assert risk[1] == 0 and not costs[1].any()
  risk.sum().backward()
  assert not torch.isnan(Wt.grad).any() and not Wt.grad[1].any() and Wt.grad[0].any()
  Wt.grad = None
  risk, costs, paths = lat.sampled_risk(_frames(B, T), torch.tensor(nf), torch.tensor(ref),
                                        torch.tensor(nl), S, 3)
  want = path_ref.edit_distance(paths.numpy(), nf, ref, nl)[0].astype(np.float32)
  want[1] = 0                                      # the unsampled utterance: costs 0, risk 0
  assert costs.dtype == torch.float32
  np.testing.assert_array_equal(costs.numpy(), want)
  np.testing.assert_array_equal(risk.detach().numpy(), want.mean(-1))
  risk.sum().backward()
  assert not torch.isnan(Wt.grad).any() and not Wt.grad[1].any()
  assert Wt.grad[0].any()
  with torch.no_grad():                            # no gradient wanted: the same values
    again = lat.sampled_risk(_frames(B, T), torch.tensor(nf), torch.tensor(ref),
                             torch.tensor(nl), S, 3)
  np.testing.assert_array_equal(again[0].numpy(), risk.detach().numpy())
  np.testing.assert_array_equal(again[2].numpy(), paths.numpy())
