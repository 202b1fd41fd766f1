"""RecognitionLattice.align_expectation on CPU tensors (cpu.align_expectation,
plain autograd) against the references of tests/align_expect_ref.py: the
enumeration of every alignment (T = 5, U = 2: 10 paths, V = 2 bigram) and
double autograd of cpu._string_distance in float64, plus the identities and
edge rules of include/lt_string_expect.h, the exports the header declares and
the host validation of the two entry points.

The CPU path runs in float32; it is held to rtol = atol = 1e-4 against the
float64 references (the project's Log parity bound), gradients included.
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
import align_expect_ref as ref
from abi_graph import dummy_graph

TOL = dict(rtol=1e-4, atol=1e-4)
HEADER_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include')


def _close(got, want):
  np.testing.assert_allclose(got.detach().double().numpy(), want.detach().double().numpy(), **TOL)


def _problem(seed, B, T, U, V=4, n=1):
  g = torch.Generator().manual_seed(seed)
  ctx = lt.contexts.FullNGram(vocab_size=V, context_size=n)
  W = torch.randn([B, T, ctx.num_states(), V + 1], generator=g)
  lab = torch.randint(1, V + 1, [B, U], generator=g)
  lv = torch.randn([B, T, U], generator=g)
  bv = torch.randn([B, T, U + 1], generator=g)
  return ctx, W, lab, lv, bv


def _call(ctx, W, nf, lab, nl, lv, bv=None, K=0, grad=False):
  table = W.clone().requires_grad_(grad)
  lat = ref.lattice(ctx, K, table)
  batch = tuple(nf.shape)
  E, lp = lat.align_expectation(ref.frames(batch, W.shape[-3]), nf, lab, nl, lv, bv)
  return table, E, lp


def test_enumeration_parity_of_values_and_all_gradients():
  T, U, V = 5, 2, 2
  ctx, W, lab, lv, bv = _problem(1, 3, T, U, V=V)
  nf, nl = torch.full([3], T), torch.full([3], U)
  a = torch.tensor([0.7, -1.3, 0.4])
  b = torch.tensor([-0.5, 0.9, 1.1])
  Wd, lvd, bvd = (x.double().requires_grad_(True) for x in (W, lv, bv))
  rows = [ref.enumerate_alignments(Wd[i], lab[i], lvd[i], bvd[i], ctx) for i in range(3)]
  E64, lp64 = torch.stack([r[0] for r in rows]), torch.stack([r[1] for r in rows])
  want = torch.autograd.grad((a.double() * E64 + b.double() * lp64).sum(), [Wd, lvd, bvd])
  lvg, bvg = lv.clone().requires_grad_(True), bv.clone().requires_grad_(True)
  table, E, lp = _call(ctx, W, nf, lab, nl, lvg, bvg, grad=True)
  assert E.dtype == torch.float32 and tuple(E.shape) == (3,) and tuple(lp.shape) == (3,)
  _close(E, E64)
  _close(lp, lp64)
  got = torch.autograd.grad((a * E + b * lp).sum(), [table, lvg, bvg])
  for x, y in zip(got, want):
    _close(x, y)
  # the string's own weights as values: log_prob - expected is the alignment entropy
  blank, lex = cpu.string_weights(W, lab, ctx)
  _, Ew, lpw = _call(ctx, W, nf, lab, nl, lex, blank)
  H = torch.stack([r[2] for r in [ref.enumerate_alignments(
      Wd[i], lab[i], lex[i].double(), blank[i].double(), ctx) for i in range(3)]])
  assert (lpw - Ew >= 0).all()
  _close(lpw - Ew, H)


def test_double_autograd_reference_parity():
  ctx, W, lab, lv, bv = _problem(2, 4, 11, 4, n=2)
  lab[0, 1] = 0  # an epsilon
  nf, nl = torch.tensor([11, 8, 1, 0]), torch.tensor([4, 2, 1, 0])
  r64 = ref.reference(W, nf, lab, nl, ctx, lv, bv)
  lvg, bvg = lv.clone().requires_grad_(True), bv.clone().requires_grad_(True)
  table, E, lp = _call(ctx, W, nf, lab, nl, lvg, bvg, grad=True)
  _close(E, r64['expected'])
  _close(lp, r64['log_prob'])
  dW, dl, db = torch.autograd.grad(E.sum(), [table, lvg, bvg], retain_graph=True)
  _close(dW, r64['dW_expected'])
  _close(dl, r64['emission'])
  _close(db, r64['blank_occ'])
  (dW,) = torch.autograd.grad(lp.sum(), [table])
  _close(dW, r64['dW_log_prob'])
  assert E[3] == 0 and lp[3] == 0  # nf = 0 with nl = 0


def test_identities():
  T, U = 12, 5
  ctx, W, lab, lv, bv = _problem(3, 3, T, U)
  nf, nl = torch.tensor([12, 9, 7]), torch.tensor([5, 3, 0])
  lat = ref.lattice(ctx, 0, W)
  fr = ref.frames((3,), T)
  # lexical_values = t: the expected emission frames, summed over the labels
  tv = torch.arange(T, dtype=torch.float32)[None, :, None].expand(3, T, U)
  E, lp = lat.align_expectation(fr, nf, lab, nl, tv)
  em, lp2 = lat.align_posteriors(fr, nf, lab, nl)
  _close(E, (torch.arange(T)[:, None] * em).sum((-2, -1)))
  _close(lp, lp2)
  # one per lexical arc counts the labels, one per blank arc the other frames
  E, _ = lat.align_expectation(fr, nf, lab, nl, torch.ones(3, T, U), torch.zeros(3, T, U + 1))
  _close(E, nl.float())
  E, _ = lat.align_expectation(fr, nf, lab, nl, torch.zeros(3, T, U), torch.ones(3, T, U + 1))
  _close(E, (nf - nl).float())
  # blank_values=None is zeros
  E0, lp0 = lat.align_expectation(fr, nf, lab, nl, lv)
  E1, lp1 = lat.align_expectation(fr, nf, lab, nl, lv, torch.zeros(3, T, U + 1))
  assert torch.equal(E0, E1) and torch.equal(lp0, lp1)
  assert not E0.requires_grad and not lp0.requires_grad


def test_every_live_frame_gradient_sums_to_zero_over_the_arcs():
  """A path takes exactly one arc per live frame, so shifting every arc of a
  frame by a constant changes no posterior: d expected / dW sums to 0 over a
  frame's arcs (and d log_prob / dW to 1)."""
  T, U = 10, 4
  ctx, W, lab, lv, bv = _problem(4, 3, T, U)
  nf, nl = torch.tensor([10, 7, 4]), torch.tensor([4, 4, 1])
  table, E, lp = _call(ctx, W, nf, lab, nl, lv, bv, grad=True)
  (dW,) = torch.autograd.grad(E.sum(), [table], retain_graph=True)
  live = torch.arange(T)[None] < nf[:, None]
  assert dW.sum((-2, -1)).abs().max() < 1e-4
  assert not dW[~live].any()
  (dW,) = torch.autograd.grad(lp.sum(), [table])
  _close(dW.sum((-2, -1)), live.float())


def test_frame_label_dependent_parity():
  ctx, W, lab, lv, bv = _problem(5, 3, 6, 7)
  nf, nl = torch.tensor([6, 4, 2]), torch.tensor([7, 7, 5])  # the last: 5 labels > 2 frames x 2
  r64 = ref.reference(W, nf, lab, nl, ctx, lv, bv, K=2)
  assert torch.isfinite(r64['log_prob'][:2]).all() and r64['log_prob'][2] == -torch.inf
  table, E, lp = _call(ctx, W, nf, lab, nl, lv, bv, K=2, grad=True)
  _close(E, r64['expected'])
  assert torch.equal(torch.isfinite(lp), torch.isfinite(r64['log_prob']))
  _close(lp[:2], r64['log_prob'][:2])
  (dW,) = torch.autograd.grad(E.sum(), [table])
  _close(dW, r64['dW_expected'])


def test_edge_rules_and_nan_values_under_minus_inf_arcs():
  T, U = 9, 3
  ctx, W, lab, lv, bv = _problem(6, 6, T, U)
  g = torch.Generator().manual_seed(60)
  W[torch.rand(W.shape, generator=g) < 0.15] = -torch.inf
  W[1, 0, 0, :] = -torch.inf                      # nothing leaves the start state: no path
  nf = torch.tensor([9, 9, 9, 2, 0, 9])
  nl = torch.tensor([3, 3, 7, 3, 0, -1])          # 2: nl > U; 3: more labels than frames; 5: nl < 0
  blank, lex = cpu.string_weights(W, lab, ctx)
  lv = torch.where(torch.isfinite(lex), lv, torch.full_like(lv, torch.nan))
  bv = torch.where(torch.isfinite(blank), bv, torch.full_like(bv, torch.nan))
  lv[3, 2:], bv[3, 2:] = torch.nan, torch.nan     # padding frames are not read
  r64 = ref.reference(W, nf, lab, nl, ctx, lv, bv)
  assert torch.isfinite(r64['log_prob'][0])       # the masked utterance stays aligned
  lvg, bvg = lv.clone().requires_grad_(True), bv.clone().requires_grad_(True)
  table, E, lp = _call(ctx, W, nf, lab, nl, lvg, bvg, grad=True)
  assert not torch.isnan(E).any() and not torch.isnan(lp).any()
  _close(E, r64['expected'])
  assert E[0] != 0
  for b in (1, 2, 3, 5):
    assert lp[b] == -torch.inf and E[b] == 0
  assert lp[4] == 0 and E[4] == 0
  fin = torch.isfinite(lp)
  grads = torch.autograd.grad((E + torch.where(fin, lp, torch.zeros_like(lp))).sum(),
                              [table, lvg, bvg])
  for x in grads:
    assert not torch.isnan(x).any()
  for b in (1, 2, 3, 4, 5):
    assert not any(x[b].any() for x in grads)
  assert not grads[0][0][~torch.isfinite(W[0])].any()
  _close(grads[1], r64['emission'])
  _close(grads[2], r64['blank_occ'])


def test_multi_dimensional_batch_dims_and_shape_errors():
  T, U = 8, 3
  ctx, W, lab, lv, bv = _problem(7, 6, T, U)
  nf, nl = torch.tensor([8, 5, 8, 3, 0, 6]), torch.tensor([3, 2, 0, 3, 0, 1])
  _, E, lp = _call(ctx, W, nf, lab, nl, lv, bv)
  shape = lambda x: x.reshape(2, 3, *x.shape[1:])
  _, E2, lp2 = _call(ctx, shape(W), shape(nf), shape(lab), shape(nl), shape(lv), shape(bv))
  assert tuple(E2.shape) == (2, 3) and tuple(lp2.shape) == (2, 3)
  assert torch.equal(E2.reshape(6), E) and torch.equal(lp2.reshape(6), lp)
  lat = ref.lattice(ctx, 0, W)
  fr = ref.frames((6,), T)
  with pytest.raises(ValueError, match='lexical_values'):
    lat.align_expectation(fr, nf, lab, nl, lv[:, :, :2], bv)
  with pytest.raises(ValueError, match='blank_values'):
    lat.align_expectation(fr, nf, lab, nl, lv, bv[:, :, :U])
  with pytest.raises(ValueError, match='lexical_values'):
    lat.align_expectation(fr, nf, lab, nl, lv[:5], bv)
  with pytest.raises(ValueError):
    lat.align_expectation(fr, nf, lab[:5], nl, lv, bv)
  with pytest.raises(ValueError):
    lat.align_expectation(fr, nf, lab, nl[:5], lv, bv)


def test_library_exports_what_lt_string_expect_h_declares():
  """include/lt_string_expect.h declares the three entry points, the library
  exports them, and lt_lattice.h includes the header."""
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(HEADER_DIR, 'lt_string_expect.h')).read(),
               flags=re.S)
  declared = sorted(set(re.findall(r'\b(lt_[a-z_]+)\s*\(', src)))
  assert declared == sorted(_native.EXPORTED_ALIGN_EXPECT)
  lib = _native.lib()
  for name in declared:
    assert hasattr(lib, name)
  assert '#include "lt_string_expect.h"' in open(os.path.join(HEADER_DIR, 'lt_lattice.h')).read()


def test_host_validation_needs_no_device():
  """Range and argument checks run on the host before anything is launched:
  FrameLabelDependent and U = 256 are LT_EUNSUPPORTED from the workspace query
  on, for both entry points; the LDS rule of include/lt_string_expect.h
  (36 SP + 12 SP T <= 160 KiB) decides between an empty workspace and
  [B, T, SP] 12-byte triples: T <= 210 / 103 / 50 at SP = 64 / 128 / 256."""
  lib = _native.lib()
  EINVAL, EUNSUPPORTED = -1, _native.LT_EUNSUPPORTED
  null = ctypes.c_void_p(0)
  # host arrays stand in for the device pointers: nothing below dereferences them
  buf = (ctypes.c_int64 * 64)()
  p = ctypes.c_void_p(ctypes.addressof(buf))
  TP = _native.TableProblem

  def graph(K=0, C=5, V=4):
    return dummy_graph(p, K, C, V)

  def query(K, T, U):
    n = ctypes.c_size_t(123)
    pb = TP(batch=4, max_frames=T, max_labels=U, weight_dtype=0)
    rc = lib.lt_table_align_expectation_workspace_bytes(ctypes.byref(graph(K)), ctypes.byref(pb),
                                                        ctypes.byref(n))
    return rc, n.value

  def call(g, pb, ptrs=None, ws=null, nbytes=0):
    ptrs = [p] * 12 if ptrs is None else ptrs
    return lib.lt_table_align_expectation(ctypes.byref(g), ctypes.byref(pb), *ptrs, ws, nbytes,
                                          null)

  def scatter(g, pb, ptrs=None):
    ptrs = [p] * 6 if ptrs is None else ptrs
    return lib.lt_table_string_scatter(ctypes.byref(g), ctypes.byref(pb), *ptrs, null)

  assert query(2, 10, 5) == (EUNSUPPORTED, 123)  # a refused query writes nothing
  assert query(0, 10, 256) == (EUNSUPPORTED, 123)
  assert query(0, 10, 255) == (0, 0)
  for U, t_lds in ((0, 210), (63, 210), (64, 103), (127, 103), (128, 50), (255, 50)):
    SP = 64 if U < 64 else (128 if U < 128 else 256)
    assert 36 * SP + 12 * SP * t_lds <= 160 * 1024 < 36 * SP + 12 * SP * (t_lds + 1)
    assert query(0, t_lds, U) == (0, 0)
    assert query(0, t_lds + 1, U) == (0, 4 * (t_lds + 1) * 12 * SP)
  ok = TP(batch=2, max_frames=4, max_labels=3, weight_dtype=0)
  long_u = TP(batch=2, max_frames=4, max_labels=256, weight_dtype=0)
  assert call(graph(), long_u) == EUNSUPPORTED and scatter(graph(), long_u) == EUNSUPPORTED
  assert call(graph(K=1), ok) == EUNSUPPORTED and scatter(graph(K=1), ok) == EUNSUPPORTED
  assert call(graph(), TP(batch=2, max_frames=4, max_labels=3, weight_dtype=5)) == EINVAL
  assert call(graph(), TP(batch=-1, max_frames=4, max_labels=3, weight_dtype=0)) == EINVAL
  for i in (0, 1, 2, 3, 4, 5, 6, 7):  # W, the values, lengths, labels, expected, log_prob
    ptrs = [p] * 12
    ptrs[i] = null
    assert call(graph(), ok, ptrs) == EINVAL, i
    assert b'null pointer' in lib.lt_last_error()
  ptrs = [p] * 12
  ptrs[9] = ctypes.c_void_p(p.value + 2)
  assert call(graph(), ok, ptrs) == EINVAL and b'misaligned' in lib.lt_last_error()
  big = TP(batch=2, max_frames=300, max_labels=3, weight_dtype=0)  # past the LDS rule
  assert call(graph(), big) == EINVAL and b'workspace' in lib.lt_last_error()
  for i in (1, 2, 4, 5):  # g_blank, num_frames, num_labels, dW
    ptrs = [p] * 6
    ptrs[i] = null
    assert scatter(graph(), ok, ptrs) == EINVAL, i
  assert call(graph(), TP(batch=0, max_frames=4, max_labels=3, weight_dtype=0), [null] * 12) == 0
  assert scatter(graph(), TP(batch=0, max_frames=4, max_labels=3, weight_dtype=0),
                 [null] * 6) == 0
