"""Prefix beam search without a GPU (RecognitionLattice.beam_search on CPU
tensors -> cpu.beam_search, the definition of include/lt_beam.h in torch ops).

* Exhaustive: with V = 2, T = 5 and K = 64 nothing is pruned, so the beam is
  all 63 label sequences of length <= 5, each scored by its string forward,
  and the scores sum to log_z; in MaxTropical the top hypothesis is
  shortest_path's.
* Pruned: beam_ref.replay judges every frame of cpu.beam_search's trace on its
  own (candidates recomputed in float64 with merges by prefix identity).
* Properties: the Log score never exceeds the string forward, K = 1 is greedy,
  ragged / empty / all -inf utterances, masked arcs, batch dims, the error
  cases, the hash, and that merging is exercised by the biased inputs.
"""
import os
import re

import numpy as np
import pytest
import torch

import last_torch_amd as lt
from last_torch_amd import _native
from last_torch_amd import cpu
import beam_ref as ref
import sample_ref

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include',
                      'lt_lattice.h')
SEMIRINGS = {'Log': lt.semirings.Log, 'MaxTropical': lt.semirings.MaxTropical}


def _lattice(context, table, K=0):
  align = lt.alignments.FrameDependent() if K == 0 else lt.alignments.FrameLabelDependent(K)
  return lt.RecognitionLattice(
      context=context, alignment=align,
      weight_fn_cacher_factory=lambda _: lt.weight_fns.NullCacher(),
      weight_fn_factory=lambda _: lt.weight_fns.TableWeightFn(table))


def _frames(B, T):
  return torch.arange(T, dtype=torch.float32)[None, :, None].expand(B, T, 1)


def _beam(context, W, nf, K, semiring):
  B, T = W.shape[:2]
  lat = _lattice(context, torch.as_tensor(W))
  labels, num_labels, scores = lat.beam_search(_frames(B, T), torch.tensor(nf), K,
                                               SEMIRINGS[semiring])
  assert labels.dtype == torch.int64 and tuple(labels.shape) == (B, K, T)
  assert num_labels.dtype == torch.int64 and tuple(num_labels.shape) == (B, K)
  assert scores.dtype == torch.float32 and tuple(scores.shape) == (B, K)
  assert not (labels.requires_grad or scores.requires_grad)
  return lat, labels, num_labels, scores


def _string_forward(lat, W, nf, labels, num_labels, semiring):
  """_string_forward of every hypothesis [B, K] (dead slots included)."""
  B, K, T = labels.shape
  lat_k = _lattice(lat.context, torch.as_tensor(W).repeat_interleave(K, dim=0))
  out = lat_k._string_forward(None, _frames(B * K, T), torch.tensor(nf).repeat_interleave(K),
                              labels.reshape(B * K, T), num_labels.reshape(B * K),
                              SEMIRINGS[semiring])
  return out.reshape(B, K)


def test_exhaustive_v2_t5():
  rng = np.random.default_rng(11)
  V, T, K = 2, 5, 64
  context = lt.contexts.FullNGram(vocab_size=V, context_size=1)
  W = ref.make_weights(rng, 1, T, V + 1, V, 1.5)
  lat, labels, nl, scores = _beam(context, W, [T], K, 'Log')
  live = scores[0] > -np.inf
  assert int(live.sum()) == 63 and bool(live[:63].all())   # 1 + 2 + ... + 32 sequences
  seqs = {tuple(labels[0, r, :nl[0, r]].tolist()) for r in range(63)}
  assert len(seqs) == 63 and all(0 not in s for s in seqs)
  assert not labels[0, 63].any() and nl[0, 63] == 0
  want = _string_forward(lat, W, [T], labels, nl, 'Log')
  np.testing.assert_allclose(scores[0, :63].numpy(), want[0, :63].numpy(), rtol=0, atol=1e-4)
  log_z, _ = lat._forward(None, _frames(1, T), torch.tensor([T]), lt.semirings.Log)
  assert abs(float(torch.logsumexp(scores[0, :63], 0)) - float(log_z[0])) <= 1e-4
  # the float64 reference agrees on the whole beam
  want_beam = ref.search(W, [T], sample_ref.table_of(context), K, 'Log')[0]
  assert {p for p, _ in want_beam} == seqs
  # MaxTropical: the top hypothesis is the best path
  _, mlab, mnl, mscores = _beam(context, W, [T], K, 'MaxTropical')
  path, _, weight = lat.shortest_path(_frames(1, T), torch.tensor([T]), label_convention='true')
  assert abs(float(mscores[0, 0]) - float(weight[0])) <= 1e-4
  assert mlab[0, 0, :mnl[0, 0]].tolist() == [y for y in path[0].tolist() if y]


PRUNED = {
    'bigram_v5': (lambda rng: lt.contexts.FullNGram(vocab_size=5, context_size=1), 4, 30),
    'trigram_v5': (lambda rng: lt.contexts.FullNGram(vocab_size=5, context_size=2), 8, 30),
    'table_c17_v6': (lambda rng: lt.contexts.NextStateTable(sample_ref.random_table(rng, 17, 6)),
                     8, 30),
}


def _pruned_case(name):
  make, K, T = PRUNED[name]
  rng = np.random.default_rng(sum(map(ord, name)))
  context = make(rng)
  table = sample_ref.table_of(context)
  C, V = table.shape
  nf = [T, T - 3, 1, 0]
  return context, table, K, T, nf, ref.make_weights(rng, 4, T, C, V, 1.5)


@pytest.mark.parametrize('semiring', list(SEMIRINGS))
@pytest.mark.parametrize('name', list(PRUNED))
def test_replay(name, semiring):
  context, table, K, T, nf, W = _pruned_case(name)
  out = cpu.beam_search(torch.tensor(W), torch.tensor(nf), context, K, SEMIRINGS[semiring],
                        want_trace=True)
  labels, nl, scores, trace, step = (x.numpy() for x in out)
  steps, final = ref.replay(W, nf, table, K, semiring, trace, step)
  assert steps == sum(nf)
  ref.check_outputs(final, trace, nf, labels, nl, scores)
  assert any(len(f) == K for f in final)   # the beam did fill: something was pruned
  # the API returns the same beam
  _, alab, anl, asc = _beam(context, W, nf, K, semiring)
  assert np.array_equal(alab.numpy(), labels) and np.array_equal(anl.numpy(), nl)
  assert np.array_equal(asc.numpy(), scores)


@pytest.mark.parametrize('name', list(PRUNED))
def test_log_score_below_string_forward_and_merging_matters(name):
  context, table, K, T, nf, W = _pruned_case(name)
  lat, labels, nl, scores = _beam(context, W, nf, K, 'Log')
  want = _string_forward(lat, W, nf, labels, nl, 'Log').numpy()
  live = scores.numpy() > -np.inf
  got = scores.numpy()
  assert (got[live] <= want[live] + (1e-4 + 1e-4 * np.abs(want[live]))).all()
  assert live[3].tolist() == [True] + [False] * (K - 1) and got[3, 0] == 0   # nf = 0
  # with the blank bias prefixes meet their parents in the beam: the (+)-sum
  # of alignments then differs from the best alignment
  _, _, _, mscores = _beam(context, W, nf, K, 'MaxTropical')
  assert abs(float(scores[0, 0]) - float(mscores[0, 0])) > 1e-2


def test_greedy_is_beam_one():
  context, table, _, T, nf, W = _pruned_case('table_c17_v6')
  for semiring in SEMIRINGS:
    _, labels, nl, scores = _beam(context, W, nf, 1, semiring)
    for b in range(4):
      c, s, seq = 0, np.float32(0), []
      for t in range(nf[b]):
        row = W[b, t, c]
        y = int(np.argmax(row))   # first maximum: the smallest y
        s = np.float32(s + row[y])
        if y:
          seq.append(y)
          c = int(table[c, y - 1])
      assert labels[b, 0, :nl[b, 0]].tolist() == seq and float(scores[b, 0]) == float(s)


def test_dead_beams_and_masked_arcs():
  rng = np.random.default_rng(5)
  context = lt.contexts.FullNGram(vocab_size=3, context_size=1)
  B, T, K = 3, 8, 6
  W = ref.make_weights(rng, B, T, 4, 3, 1.5)
  W[1] = -np.inf                        # no arc at all: an all-dead beam
  W[2, :, :, 2] = -np.inf               # label 2 masked everywhere
  W[2, 3, :, 0] = -np.inf               # and no blank on frame 3
  for semiring in SEMIRINGS:
    _, labels, nl, scores = _beam(context, W, [T, T, T], K, semiring)
    assert (scores[1] == -np.inf).all() and not labels[1].any() and not nl[1].any()
    assert np.isfinite(scores[[0, 2]].numpy()).all()
    assert (labels[2] != 2).all() and (nl[2] >= 1).all()
    out = cpu.beam_search(torch.tensor(W), torch.tensor([T, T, T]), context, K,
                          SEMIRINGS[semiring], want_trace=True)
    steps, _ = ref.replay(W, [T, T, T], sample_ref.table_of(context), K, semiring,
                          out[3].numpy(), out[4].numpy())
    assert steps == 3 * T


def test_batch_dims():
  rng = np.random.default_rng(6)
  context = lt.contexts.FullNGram(vocab_size=3, context_size=1)
  W = torch.tensor(ref.make_weights(rng, 6, 5, 4, 3, 1.5).reshape(2, 3, 5, 4, 4))
  lat = _lattice(context, W)
  frames = torch.arange(5, dtype=torch.float32)[:, None].expand(2, 3, 5, 1)
  nf = torch.tensor([[5, 4, 3], [2, 1, 0]])
  labels, nl, scores = lat.beam_search(frames, nf, 4)
  assert tuple(labels.shape) == (2, 3, 4, 5) and tuple(nl.shape) == (2, 3, 4)
  assert tuple(scores.shape) == (2, 3, 4)
  _, flab, fnl, fsc = _beam(context, W.reshape(6, 5, 4, 4).numpy(), nf.reshape(-1).tolist(), 4,
                            'Log')
  assert torch.equal(labels.reshape(6, 4, 5), flab) and torch.equal(nl.reshape(6, 4), fnl)
  assert torch.equal(scores.reshape(6, 4), fsc)
  # labels + num_frames are edit_distance hypotheses as they are
  dist = lt.edit_distance(labels, nf, labels[..., 0, :], nl[..., 0])
  assert tuple(dist.shape) == (2, 3, 4) and (dist[..., 0] == 0).all()
  assert (dist[0, 0, 1:] > 0).all()   # the other hypotheses differ from the best


def test_error_cases():
  context = lt.contexts.FullNGram(vocab_size=3, context_size=1)
  frames, nf = torch.zeros([1, 4, 1]), torch.tensor([4])
  with pytest.raises(NotImplementedError):
    _lattice(context, torch.zeros([1, 4, 4, 4]), K=2).beam_search(frames, nf, 4)
  lat = _lattice(context, torch.zeros([1, 4, 4, 4]))
  with pytest.raises(ValueError):
    lat.beam_search(frames, nf, 0)
  with pytest.raises(NotImplementedError):
    lat.beam_search(frames, nf, 4, semiring=lt.semirings.Real)


def test_prefix_hash_matches_python_integers():
  M = (1 << 64) - 1

  def mix(h, y):
    z = h ^ ((y * 0x9E3779B97F4A7C15) & M)
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return z ^ (z >> 31)

  h = 0
  for y in [1, 32, 7, 1023, 1, 1]:
    want = mix(h, y)
    got = int(cpu.prefix_hash(torch.tensor([cpu._i64(h)]), torch.tensor([y]))[0]) & M
    assert got == want
    h = want


def test_library_exports_what_lt_beam_h_declares():
  """include/lt_beam.h declares the two entry points, the library exports
  them, the binding lists them, and lt_lattice.h pulls the header in."""
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(os.path.dirname(HEADER), 'lt_beam.h')).read(),
               flags=re.S)
  declared = sorted(set(re.findall(r'\b(lt_[a-z_]+)\s*\(', src)))
  assert declared == sorted(_native.EXPORTED_BEAM) and len(declared) == 2
  for name in declared:
    assert hasattr(_native.lib(), name) and name in _native._SIG
  assert '#include "lt_beam.h"' in open(HEADER).read()
