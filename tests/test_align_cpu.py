"""Forced alignment without a GPU.

* RecognitionLattice.align on CPU tensors (cpu.align) against the reference's
  own autograd through _string_forward in MaxTropical (tests/golden/grads_*),
  compacted by align_compact.compact: every FrameDependent and
  FrameLabelDependent fixture (epsilons, integer ties, unreachable strings),
  all three outputs exact and the weights bit-equal to num_MaxTropical.
* lt_table_align's host validation: error codes come back before any device
  work, so they are checked here (as test_host_validation_error_codes does).
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import last_torch_amd as lt
from last_torch_amd import _native
from align_compact import CASES, compact, load
from abi_graph import dummy_graph

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include',
                      'lt_lattice.h')


def _lattice(context, K, table):
  align = lt.alignments.FrameDependent() if K == 0 else lt.alignments.FrameLabelDependent(K)
  return lt.RecognitionLattice(
      context=context, alignment=align,
      weight_fn_cacher_factory=lambda _: lt.weight_fns.NullCacher(),
      weight_fn_factory=lambda _: lt.weight_fns.TableWeightFn(table))


def test_fixture_count():
  assert len(CASES) == 25


@pytest.mark.parametrize('name', CASES)
def test_cpu_align_matches_reference_autograd(name):
  d = load(name)
  V, n, K = int(d['vocab_size']), int(d['context_size']), d['K']
  B, T = d['W'].shape[:2]
  ref_labels, ref_frames = compact(d['num_grad_MaxTropical'], d['num_MaxTropical'], d['labels'],
                                   d['num_labels'], d['num_frames'], K)
  lat = _lattice(lt.contexts.FullNGram(vocab_size=V, context_size=n), K, torch.tensor(d['W']))
  frames = torch.arange(T, dtype=torch.float32)[None, :, None].expand(B, T, 1)
  got_labels, got_frames, got_w = lat.align(frames, torch.tensor(d['num_frames']),
                                            torch.tensor(d['labels']), torch.tensor(d['num_labels']))
  assert got_labels.dtype == torch.int64 and got_frames.dtype == torch.int64
  assert tuple(got_labels.shape) == (B, T * (K + 1 if K else 1))
  np.testing.assert_array_equal(got_w.numpy(), d['num_MaxTropical'])
  np.testing.assert_array_equal(got_labels.numpy(), ref_labels)
  np.testing.assert_array_equal(got_frames.numpy(), ref_frames)


def _define(name):
  return int(re.search(rf'#define\s+{name}\s+\(?(-?\d+)\)?', open(HEADER).read()).group(1))


def test_library_exports_what_lt_align_h_declares():
  """include/lt_align.h declares the two alignment entry points, the library
  exports them, the binding lists them, and lt_lattice.h pulls the header in."""
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(os.path.dirname(HEADER), 'lt_align.h')).read(),
               flags=re.S)
  declared = sorted(set(re.findall(r'\b(lt_[a-z_]+)\s*\(', src)))
  assert declared == sorted(_native.EXPORTED_ALIGN) and len(declared) == 2
  for name in declared:
    assert hasattr(_native.lib(), name) and name in _native._SIG
  assert '#include "lt_align.h"' in open(HEADER).read()


def test_align_host_validation_error_codes():
  lib = _native.lib()
  EINVAL, EUNSUPPORTED = _define('LT_EINVAL'), _define('LT_EUNSUPPORTED')
  null = ctypes.c_void_p(0)
  # host arrays stand in for the device pointers: nothing below dereferences them
  buf = (ctypes.c_int64 * 64)()
  p = ctypes.c_void_p(ctypes.addressof(buf))

  def graph(**kw):
    return dummy_graph(p, **kw)

  def call(g, pb, W=p, nf=p, lab=p, nl=p, out=p, fr=p, w=p, ws=null, nbytes=0):
    return lib.lt_table_align(ctypes.byref(g), ctypes.byref(pb), W, nf, lab, nl, out, fr, w, ws,
                              nbytes, null)

  TP = _native.TableProblem
  ok = TP(batch=2, max_frames=4, max_labels=3, weight_dtype=0)
  assert lib.lt_table_align(None, ctypes.byref(ok), p, p, p, p, p, p, p, null, 0, null) == EINVAL
  assert call(graph(), ok, W=null) == EINVAL
  assert b'null pointer' in lib.lt_last_error()
  assert call(graph(), ok, w=null) == EINVAL
  assert b'null pointer' in lib.lt_last_error()
  assert call(graph(), ok, out=ctypes.c_void_p(p.value + 4)) == EINVAL
  assert b'misaligned' in lib.lt_last_error()
  assert call(graph(), TP(batch=-1, max_frames=4, max_labels=3, weight_dtype=0)) == EINVAL
  assert call(graph(), TP(batch=2, max_frames=4, max_labels=3, weight_dtype=5)) == EINVAL
  nbytes = ctypes.c_size_t(7)
  long_u = TP(batch=2, max_frames=4, max_labels=256, weight_dtype=0)
  assert call(graph(), long_u) == EUNSUPPORTED
  assert lib.lt_table_align_workspace_bytes(ctypes.byref(graph()), ctypes.byref(long_u),
                                            ctypes.byref(nbytes)) == EUNSUPPORTED
  assert call(graph(K=16), ok) == EUNSUPPORTED
  assert call(graph(K=15), TP(batch=0, max_frames=4, max_labels=255, weight_dtype=0),
              W=null, w=null) == 0
  # the bench shape: decisions stay in LDS, no workspace
  bench = TP(batch=64, max_frames=1000, max_labels=100, weight_dtype=0)
  assert lib.lt_table_align_workspace_bytes(ctypes.byref(graph()), ctypes.byref(bench),
                                            ctypes.byref(nbytes)) == 0
  assert nbytes.value == 0
  # beyond LDS: one 64-bit word per frame and 64 positions, per utterance
  deep = TP(batch=2, max_frames=5200, max_labels=255, weight_dtype=0)
  assert lib.lt_table_align_workspace_bytes(ctypes.byref(graph()), ctypes.byref(deep),
                                            ctypes.byref(nbytes)) == 0
  assert nbytes.value >= 2 * 5200 * 4 * 8
  assert call(graph(), deep, ws=null) == EINVAL
  assert b'workspace' in lib.lt_last_error()
