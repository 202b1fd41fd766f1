"""Path sampling without a GPU (RecognitionLattice.sample on CPU tensors ->
cpu.sample, the definition of include/lt_sample.h in torch ops).

* Philox4x32-10: Random123's known answers, for the torch implementation and
  for the independent NumPy one the replays use (sample_ref.philox).
* Exact distribution: every path of two small lattices is enumerated in
  float64 and its count among S = 8192 samples must lie within
  5 (sqrt(S p (1 - p)) + 1) of S p: five standard deviations of a binomial
  count, plus one for its discreteness (cpu.sample reaches 1.95 and 2.12).
* Validity and weight: the labels walk the next-state table from state 0 and
  path_weights equals the float64 sum of W along them within
  T 2^-23 sum |w_arc|, the fp32 summation bound.
* Determinism, the S-prefix property, ragged / empty / unsampled utterances,
  masked arcs, FrameLabelDependent, and lt_table_sample's host validation.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import last_torch_amd as lt
from last_torch_amd import _native
from last_torch_amd import cpu
import sample_ref as ref
from abi_graph import dummy_graph

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include',
                      'lt_lattice.h')


def _lattice(context, table, K=0):
  align = lt.alignments.FrameDependent() if K == 0 else lt.alignments.FrameLabelDependent(K)
  return lt.RecognitionLattice(
      context=context, alignment=align,
      weight_fn_cacher_factory=lambda _: lt.weight_fns.NullCacher(),
      weight_fn_factory=lambda _: lt.weight_fns.TableWeightFn(table))


def _sample(context, W, nf, S, seed):
  B, T = W.shape[:2]
  lat = _lattice(context, torch.as_tensor(W))
  frames = torch.arange(T, dtype=torch.float32)[None, :, None].expand(B, T, 1)
  labels, weights, log_z = lat.sample(frames, torch.tensor(nf), S, seed)
  assert labels.dtype == torch.int64 and tuple(labels.shape) == (B, S, T)
  assert tuple(weights.shape) == (B, S) and tuple(log_z.shape) == (B,)
  return labels.numpy(), weights.numpy(), log_z.numpy()


@pytest.mark.parametrize('impl', ['torch', 'numpy'])
def test_philox_known_answers(impl):
  for counter, key, out in ref.PHILOX_KAT:
    if impl == 'torch':
      got = cpu.philox4x32([torch.tensor([c]) for c in counter], [torch.tensor(k) for k in key])
    else:
      got = ref.philox([np.array([c]) for c in counter], key)
    assert tuple(int(x[0]) for x in got) == out


def test_noise_matches_the_float64_definition():
  """cpu.sample_noise (fp32) against sample_ref.noise (float64) on 40,000
  arcs: word selection k & 3, the counter layout and both halves of u."""
  k = np.arange(40000)
  got = cpu.sample_noise(0x123456789abcdef, 3, torch.tensor(5), 7, torch.tensor(k)).numpy()
  want = ref.noise(0x123456789abcdef, 3, 5, 7, k)
  assert got.dtype == np.float32
  np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-6)
  assert np.isfinite(got).all()


@pytest.mark.parametrize('name', list(ref.DISTRIBUTIONS))
def test_exact_distribution(name):
  assert ref.distribution_units(lambda *a: _sample(*a)[0], name) <= 5


@pytest.mark.parametrize('kind', ['bigram', 'trigram', 'table'])
def test_paths_are_valid_and_weights_are_their_sums(kind):
  rng = np.random.default_rng(11)
  context = {'bigram': lambda: lt.contexts.FullNGram(vocab_size=4, context_size=1),
             'trigram': lambda: lt.contexts.FullNGram(vocab_size=3, context_size=2),
             'table': lambda: lt.contexts.NextStateTable(ref.random_table(rng, 7, 3))}[kind]()
  table = ref.table_of(context)
  C, V = table.shape
  B, T, S = 5, 9, 6
  nf = [T, T - 3, 1, 0, T + 4]   # ragged, 1, 0 and one past T (clamped)
  W = rng.standard_normal([B, T, C, V + 1]).astype(np.float32)
  labels, weights, log_z = _sample(context, W, nf, S, 5)
  ref.check_paths(W, nf, table, labels, weights, log_z)
  want_z, _ = ref.forward(W, np.clip(nf, 0, T), table)
  np.testing.assert_allclose(log_z, want_z, rtol=1e-4, atol=1e-4)
  assert not weights[3].any() and not labels[3].any()  # the empty path: weight 0


def test_determinism_and_sample_prefix():
  rng = np.random.default_rng(3)
  context = lt.contexts.FullNGram(vocab_size=5, context_size=1)
  B, T = 3, 12
  W = rng.standard_normal([B, T, 6, 6]).astype(np.float32)
  nf = [T, 7, 12]
  a = _sample(context, W, nf, 8, 99)
  b = _sample(context, W, nf, 8, 99)
  c = _sample(context, W, nf, 8, 100)
  d = _sample(context, W, nf, 32, 99)
  np.testing.assert_array_equal(a[0], b[0])
  np.testing.assert_array_equal(a[1], b[1])
  assert (a[0] != c[0]).any()
  np.testing.assert_array_equal(a[0], d[0][:, :8])
  np.testing.assert_array_equal(a[1], d[1][:, :8])
  assert len({tuple(r) for r in d[0][0]}) > 1  # the samples of a call differ


def test_high_seed_bits_matter():
  rng = np.random.default_rng(4)
  context = lt.contexts.FullNGram(vocab_size=5, context_size=1)
  W = rng.standard_normal([1, 12, 6, 6]).astype(np.float32)
  a = _sample(context, W, [12], 8, 1)
  b = _sample(context, W, [12], 8, 1 + (1 << 32))
  assert (a[0] != b[0]).any()


def test_unsampled_and_masked_arcs():
  rng = np.random.default_rng(5)
  context = lt.contexts.FullNGram(vocab_size=3, context_size=1)
  table = ref.table_of(context)
  B, T, S = 3, 8, 64
  W = rng.standard_normal([B, T, 4, 4]).astype(np.float32)
  W[1] = -np.inf                        # no path at all: unsampled
  W[2, :, :, 2] = -np.inf               # label 2 masked everywhere
  W[2, 3, :, 0] = -np.inf               # and no blank on frame 3
  labels, weights, log_z = _sample(context, W, [T, T, T], S, 17)
  ref.check_paths(W, [T, T, T], table, labels, weights, log_z)
  assert log_z[1] == -np.inf and (weights[1] == -np.inf).all() and not labels[1].any()
  assert np.isfinite(weights[[0, 2]]).all()
  assert (labels[2] != 2).all() and (labels[2, :, 3] != 0).all()
  assert (labels[0] == 2).any()


def test_frame_label_dependent_raises():
  context = lt.contexts.FullNGram(vocab_size=3, context_size=1)
  lat = _lattice(context, torch.zeros([1, 4, 4, 4]), K=2)
  frames = torch.zeros([1, 4, 1])
  with pytest.raises(NotImplementedError):
    lat.sample(frames, torch.tensor([4]), 2, 0)


def test_num_samples_is_checked():
  context = lt.contexts.FullNGram(vocab_size=3, context_size=1)
  lat = _lattice(context, torch.zeros([1, 4, 4, 4]))
  with pytest.raises(ValueError):
    lat.sample(torch.zeros([1, 4, 1]), torch.tensor([4]), 0, 0)


def test_batch_dims():
  rng = np.random.default_rng(6)
  context = lt.contexts.FullNGram(vocab_size=3, context_size=1)
  W = torch.tensor(rng.standard_normal([2, 3, 5, 4, 4]).astype(np.float32))
  lat = _lattice(context, W)
  frames = torch.arange(5, dtype=torch.float32)[:, None].expand(2, 3, 5, 1)
  nf = torch.tensor([[5, 4, 3], [2, 1, 0]])
  labels, weights, log_z = lat.sample(frames, nf, 4, 8)
  assert tuple(labels.shape) == (2, 3, 4, 5) and tuple(weights.shape) == (2, 3, 4)
  assert tuple(log_z.shape) == (2, 3)
  flat = _sample(context, W.reshape(6, 5, 4, 4).numpy(), nf.reshape(-1).tolist(), 4, 8)
  np.testing.assert_array_equal(labels.reshape(6, 4, 5).numpy(), flat[0])


def _define(name):
  return int(re.search(rf'#define\s+{name}\s+\(?(-?\d+)\)?', open(HEADER).read()).group(1))


def test_library_exports_what_lt_sample_h_declares():
  """include/lt_sample.h declares the two sampling entry points, the library
  exports them, the binding lists them, and lt_lattice.h pulls the header in."""
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(os.path.dirname(HEADER), 'lt_sample.h')).read(),
               flags=re.S)
  declared = sorted(set(re.findall(r'\b(lt_[a-z_]+)\s*\(', src)))
  assert declared == sorted(_native.EXPORTED_SAMPLE) and len(declared) == 2
  for name in declared:
    assert hasattr(_native.lib(), name) and name in _native._SIG
  assert '#include "lt_sample.h"' in open(HEADER).read()


def test_sample_host_validation_error_codes():
  lib = _native.lib()
  EINVAL, EUNSUPPORTED = _define('LT_EINVAL'), _define('LT_EUNSUPPORTED')
  null = ctypes.c_void_p(0)
  # host arrays stand in for the device pointers: nothing below dereferences them
  buf = (ctypes.c_int64 * 64)()
  p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)

  def graph(**kw):
    return dummy_graph(p, **kw)

  def call(g, pb, W=p, nf=p, lz=p, al=p, S=4, out=p, w=p):
    return lib.lt_table_sample(ctypes.byref(g), ctypes.byref(pb), W, nf, lz, al, S, 1, out, w,
                               null, 0, null)

  TP = _native.TableProblem
  ok = TP(batch=2, max_frames=4, max_labels=0, weight_dtype=0)
  nbytes = ctypes.c_size_t(7)
  assert lib.lt_table_sample(None, ctypes.byref(ok), p, p, p, p, 4, 1, p, p, null, 0,
                             null) == EINVAL
  assert call(graph(), ok, S=0) == EINVAL
  assert b'num_samples' in lib.lt_last_error()
  assert lib.lt_table_sample_workspace_bytes(ctypes.byref(graph()), ctypes.byref(ok), 0,
                                             ctypes.byref(nbytes)) == EINVAL
  assert call(graph(), ok, out=null) == EINVAL
  assert b'null output' in lib.lt_last_error()
  assert call(graph(), ok, w=null) == EINVAL
  assert call(graph(), ok, al=null) == EINVAL
  assert call(graph(), ok, W=ctypes.c_void_p(p.value + 4)) == EINVAL
  assert b'misaligned' in lib.lt_last_error()
  assert call(graph(), TP(batch=2, max_frames=4, max_labels=0, weight_dtype=5)) == EINVAL
  assert call(graph(K=1), ok) == EUNSUPPORTED
  assert lib.lt_table_sample_workspace_bytes(ctypes.byref(graph(K=2)), ctypes.byref(ok), 4,
                                             ctypes.byref(nbytes)) == EUNSUPPORTED
  assert call(graph(), TP(batch=0, max_frames=4, max_labels=0, weight_dtype=0), W=null,
              al=null) == 0
  bench = TP(batch=64, max_frames=1000, max_labels=0, weight_dtype=0)
  assert lib.lt_table_sample_workspace_bytes(ctypes.byref(graph()), ctypes.byref(bench), 16,
                                             ctypes.byref(nbytes)) == 0
  assert nbytes.value == 0
