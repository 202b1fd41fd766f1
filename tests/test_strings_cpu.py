"""RecognitionLattice.string_weights / nbest_risk on the host (the torch
restatement cpu.string_scores of include/lt_strings.h): against
_string_forward(..., Log) called once per hypothesis, and nbest_risk against
the enumeration of a lattice small enough to list every label sequence."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

import last_torch_amd as lt
from last_torch_amd import _native

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include')


def _lattice(V, table):
  return lt.RecognitionLattice(
      context=lt.contexts.FullNGram(vocab_size=V, context_size=1),
      alignment=lt.alignments.FrameDependent(),
      weight_fn_cacher_factory=lambda _: lt.weight_fns.NullCacher(),
      weight_fn_factory=lambda _: lt.weight_fns.TableWeightFn(table))


def _frames(B, T):
  return torch.arange(T, dtype=torch.float32)[:, None].expand(B, T, 1)


def test_string_weights_equal_string_forward_per_hypothesis():
  V, B, N, T, U = 4, 2, 3, 6, 3
  rng = np.random.default_rng(5)
  W = torch.tensor(rng.standard_normal((B, T, V + 1, V + 1)), dtype=torch.float32,
                   requires_grad=True)
  lat = _lattice(V, W)
  nf = torch.tensor([6, 4])
  lab = torch.tensor(rng.integers(0, V + 1, (B, N, U)))
  nl = torch.tensor([[3, 0, 2], [1, 4, -1]])  # 4 and -1 lie outside [0, U]: -inf
  coef = torch.tensor(rng.standard_normal((B, N)), dtype=torch.float32)
  got = lat.string_weights(_frames(B, T), nf, lab, nl)
  assert tuple(got.shape) == (B, N)
  gW, = torch.autograd.grad((torch.where(torch.isfinite(got), got, 0 * coef) * coef).sum(), [W])
  want = torch.stack([lat._string_forward(None, _frames(B, T), nf, lab[:, n], nl[:, n],
                                          lt.semirings.Log) for n in range(N)], dim=1)
  assert torch.equal(torch.isfinite(got), torch.tensor([[True] * 3, [True, False, False]]))
  assert (got[1, 1:] == -torch.inf).all()
  torch.testing.assert_close(got, want, rtol=0, atol=1e-5)
  wW, = torch.autograd.grad((torch.where(torch.isfinite(want), want, 0 * coef) * coef).sum(), [W])
  assert torch.isfinite(gW).all() and (gW[1, 4:] == 0).all()
  torch.testing.assert_close(gW, wW, rtol=0, atol=1e-5)
  with pytest.raises(ValueError):
    lat.string_weights(_frames(B, T), nf, lab[:, 0], nl)


def test_nbest_risk_equals_the_enumerated_expectation():
  """V = 2, T = 4: the 31 label sequences of length <= 4 are every hypothesis
  the lattice gives weight to, so the posteriors sum to 1 and the risk is the
  expectation of the cost under exp(weight) / sum."""
  V, T, U = 2, 4, 4
  rng = np.random.default_rng(11)
  W = torch.tensor(rng.standard_normal((1, T, V + 1, V + 1)), dtype=torch.float64,
                   requires_grad=True)
  lat = _lattice(V, W)
  seqs = [s for k in range(U + 1) for s in itertools.product(range(1, V + 1), repeat=k)]
  hyp = torch.tensor([list(s) + [0] * (U - len(s)) for s in seqs])[None]
  hnl = torch.tensor([len(s) for s in seqs])[None]
  ref, rnl = torch.tensor([[1, 2, 2, 0]]), torch.tensor([3])
  frames, nf = _frames(1, T), torch.tensor([T])
  risk, costs, post = lat.nbest_risk(frames, nf, ref, rnl, hyp, hnl)
  g, = torch.autograd.grad(risk.sum(), [W])
  want_c = lt.edit_distance(hyp, None, ref, rnl).float()
  assert torch.equal(costs, want_c) and costs[0, seqs.index((1, 2, 2))] == 0
  # the enumeration: every sequence's weight from _string_forward in float64
  w = torch.stack([lat._string_forward(None, frames.double(), nf, hyp[:, n], hnl[:, n],
                                       lt.semirings.Log) for n in range(len(seqs))], dim=1)
  log_z = lat._forward(None, frames.double(), nf, lt.semirings.Log)[0]
  torch.testing.assert_close(torch.logsumexp(w, dim=-1), log_z.to(w.dtype), rtol=0, atol=1e-5)
  p = torch.softmax(w.double(), dim=-1)
  want = (p * want_c.double()).sum(-1)
  wg, = torch.autograd.grad(want.sum(), [W])
  assert abs(float(post.detach().sum()) - 1) < 1e-5
  torch.testing.assert_close(post.double(), p.detach(), rtol=0, atol=1e-5)
  torch.testing.assert_close(risk.double(), want.detach(), rtol=0, atol=1e-5)
  torch.testing.assert_close(g, wg, rtol=0, atol=1e-5)
  # a masked slot (hyp_num_labels = -1) drops out; given costs replace the default
  hnl2 = hnl.clone()
  hnl2[0, 0] = -1
  r2, c2, p2 = lat.nbest_risk(frames, nf, ref, rnl, hyp, hnl2, costs=torch.ones(1, len(seqs)))
  assert p2[0, 0] == 0 and abs(float(r2.detach()) - 1) < 1e-5 and (c2 == 1).all()


def test_library_exports_what_lt_strings_h_declares():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(INCLUDE, 'lt_strings.h')).read(), flags=re.S)
  declared = sorted(set(re.findall(r'\b(lt_[a-z_]+)\s*\(', src)))
  assert declared == sorted(_native.EXPORTED_STRINGS) and len(declared) == 3
  for name in declared:
    assert hasattr(_native.lib(), name) and name not in _native.EXPORTED
  assert '#include "lt_strings.h"' in open(os.path.join(INCLUDE, 'lt_lattice.h')).read()
  # the range is refused on the host, before any pointer is looked at
  graph = _native.TableGraph(lt.contexts.FullNGram(4, 1).next_state_table(), 0, 'cpu')
  pb = _native.TableProblem(2, 6, 256, _native.LT_DTYPE_F32)
  nb = _native.ctypes.c_size_t(0)
  q = _native.lib().lt_table_strings_workspace_bytes
  assert q(_native.ctypes.byref(graph.g), _native.ctypes.byref(pb), 4, _native.ctypes.byref(nb)) == -2
  pb.max_labels = 255
  assert q(_native.ctypes.byref(graph.g), _native.ctypes.byref(pb), 65, _native.ctypes.byref(nb)) == -2
  assert q(_native.ctypes.byref(graph.g), _native.ctypes.byref(pb), 64, _native.ctypes.byref(nb)) == 0
  assert nb.value >= 8 * 2 * 64 * 6 * 256
