"""RecognitionLattice.expectation without a GPU (CPU tensors -> cpu.expectation,
the definition of include/lt_expect.h by double backward through
cpu.den_forward).

* Against a float64 enumeration of every path (expect_ref.enumerate_bigram):
  E, log_z and the gradients w.r.t. W and values at 1e-10 in float64 --
  ragged lengths down to 0, one -inf arc with a NaN value on it. The same in
  float32 at the project's Log parity bound, rtol = atol = 1e-4.
* The public API: shapes, batch dims, FrameLabelDependent and a wrong values
  shape, entropy(differentiable=True), the gradient of a leaf table.
* lt_expect.h, the exports and lt_table_expectation's host validation.
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
import expect_ref as ref
from abi_graph import dummy_graph

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include',
                      'lt_lattice.h')
V, T, B = 2, 5, 4
NF = [5, 3, 1, 0]
MASKED = (0, 2, 1, 2)  # (b, t, p, y): on live paths of utterance 0


def _inputs(dtype=torch.float64, seed=0):
  g = torch.Generator().manual_seed(seed)
  W = torch.randn([B, T, V + 1, V + 1], generator=g, dtype=torch.float64)
  v = torch.randn([B, T, V + 1, V + 1], generator=g, dtype=torch.float64)
  W[MASKED] = -torch.inf
  v[MASKED] = torch.nan
  return W.to(dtype), v.to(dtype)


@pytest.fixture(scope='module')
def enumeration():
  """E, log_z, H and the gradients of E.sum(), log_z.sum() and H.sum() by
  enumeration (float64), computed once."""
  W, v = _inputs()
  W.requires_grad_(True)
  v.requires_grad_(True)
  E, log_z, H = ref.enumerate_bigram(W, v, NF)
  dE_dW, dE_dv = torch.autograd.grad(E.sum(), [W, v], retain_graph=True)
  (dZ_dW,) = torch.autograd.grad(log_z.sum(), [W], retain_graph=True)
  (dH_dW,) = torch.autograd.grad(H.sum(), [W])
  assert torch.isfinite(dE_dW).all() and torch.isfinite(dE_dv).all()
  return {k: x.detach().numpy() for k, x in
          dict(E=E, log_z=log_z, H=H, dE_dW=dE_dW, dE_dv=dE_dv, dZ_dW=dZ_dW, dH_dW=dH_dW).items()}


@pytest.mark.parametrize('dtype,tol', [(torch.float64, 1e-10), (torch.float32, 1e-4)])
def test_cpu_expectation_matches_the_enumeration(enumeration, dtype, tol):
  W, v = _inputs(dtype)
  W.requires_grad_(True)
  v.requires_grad_(True)
  context = lt.contexts.FullNGram(vocab_size=V, context_size=1)
  E, log_z = cpu.expectation(W, v, torch.tensor(NF), context)
  assert E.dtype == dtype and tuple(E.shape) == (B,) and tuple(log_z.shape) == (B,)
  dE_dW, dE_dv = torch.autograd.grad(E.sum(), [W, v], retain_graph=True)
  (dZ_dW,) = torch.autograd.grad(log_z.sum(), [W])
  got = dict(E=E, log_z=log_z, dE_dW=dE_dW, dE_dv=dE_dv, dZ_dW=dZ_dW)
  for k, x in got.items():
    np.testing.assert_allclose(x.detach().double().numpy(), enumeration[k], rtol=tol, atol=tol,
                               err_msg=k)
  assert E[3] == 0 and log_z[3] == 0                       # num_frames = 0
  assert dE_dW[MASKED] == 0 and dE_dv[MASKED] == 0         # the masked arc
  assert not dE_dW[1, 3:].any() and not dE_dv[1, 3:].any()  # padding frames


def test_unreachable_utterance_gives_zero():
  """Every arc out of the start state at -inf on frame 0: log_z = -inf,
  E = 0, zero gradients, and the other utterance is untouched."""
  W, v = _inputs()
  W, v = W[:2].clone(), torch.nan_to_num(v[:2].clone())
  W[1, 0, 0, :] = -torch.inf
  W.requires_grad_(True)
  v.requires_grad_(True)
  context = lt.contexts.FullNGram(vocab_size=V, context_size=1)
  E, log_z = cpu.expectation(W, v, torch.tensor([T, T]), context)
  assert log_z[1] == -torch.inf and E[1] == 0 and torch.isfinite(E[0])
  dW, dv = torch.autograd.grad(E.sum(), [W, v])
  assert not dW[1].any() and not dv[1].any()
  assert torch.isfinite(dW).all() and torch.isfinite(dv).all() and dW[0].any()


def test_public_api_matches_cpu_expectation_and_batch_dims():
  W, v = _inputs(torch.float32)
  context = lt.contexts.FullNGram(vocab_size=V, context_size=1)
  lat = ref.table_lattice(context, W)
  nf = torch.tensor(NF)
  E, log_z = lat.expectation(ref.frames([B], T), nf, v)
  assert tuple(E.shape) == (B,) and tuple(log_z.shape) == (B,)
  wantE, wantZ = cpu.expectation(W, v, nf, context)
  np.testing.assert_array_equal(E.numpy(), wantE.numpy())
  np.testing.assert_array_equal(log_z.numpy(), wantZ.numpy())
  # batch dims [2, 2]
  lat2 = ref.table_lattice(context, W.reshape(2, 2, T, V + 1, V + 1))
  E2, Z2 = lat2.expectation(ref.frames([2, 2], T), nf.reshape(2, 2),
                            v.reshape(2, 2, T, V + 1, V + 1))
  assert tuple(E2.shape) == (2, 2) and tuple(Z2.shape) == (2, 2)
  np.testing.assert_array_equal(E2.reshape(-1).numpy(), E.numpy())
  np.testing.assert_array_equal(Z2.reshape(-1).numpy(), log_z.numpy())


def test_frame_label_dependent_and_wrong_shape_raise():
  context = lt.contexts.FullNGram(vocab_size=V, context_size=1)
  W = torch.zeros([1, T, V + 1, V + 1])
  with pytest.raises(NotImplementedError):
    ref.table_lattice(context, W, K=2).expectation(ref.frames([1], T), torch.tensor([T]), W)
  with pytest.raises(NotImplementedError):
    ref.table_lattice(context, W, K=2).entropy(ref.frames([1], T), torch.tensor([T]),
                                               differentiable=True)
  lat = ref.table_lattice(context, W)
  with pytest.raises(ValueError):
    lat.expectation(ref.frames([1], T), torch.tensor([T]), W[..., :V])
  with pytest.raises(ValueError):
    lat.expectation(ref.frames([1], T), torch.tensor([T]), W[0])


def test_differentiable_entropy(enumeration):
  W, _ = _inputs(torch.float32)
  table = W.clone().requires_grad_(True)
  context = lt.contexts.FullNGram(vocab_size=V, context_size=1)
  lat = ref.table_lattice(context, table)
  nf = torch.tensor(NF)
  H = lat.entropy(ref.frames([B], T), nf, differentiable=True)
  assert H.requires_grad
  H0 = lat.entropy(ref.frames([B], T), nf)
  assert not H0.requires_grad
  np.testing.assert_allclose(H.detach().numpy(), H0.numpy(), rtol=1e-5, atol=1e-5)
  np.testing.assert_allclose(H.detach().numpy(), enumeration['H'], rtol=1e-4, atol=1e-4)
  (dH,) = torch.autograd.grad(H.sum(), [table])
  np.testing.assert_allclose(dH.numpy(), enumeration['dH_dW'], rtol=1e-4, atol=1e-4)


def test_leaf_table_receives_the_gradient(enumeration):
  W, v = _inputs(torch.float32)
  table = W.clone().requires_grad_(True)
  context = lt.contexts.FullNGram(vocab_size=V, context_size=1)
  E, log_z = ref.table_lattice(context, table).expectation(ref.frames([B], T), torch.tensor(NF), v)
  (E.sum() + log_z.sum()).backward()
  assert table.grad is not None and table.grad.shape == table.shape
  np.testing.assert_allclose(table.grad.numpy(), enumeration['dE_dW'] + enumeration['dZ_dW'],
                             rtol=1e-4, atol=1e-4)


def test_no_grad_inputs_give_plain_values():
  W, v = _inputs(torch.float32)
  context = lt.contexts.FullNGram(vocab_size=V, context_size=1)
  E, log_z = cpu.expectation(W, v, torch.tensor(NF), context)
  assert not E.requires_grad and not log_z.requires_grad


def _define(name):
  return int(re.search(rf'#define\s+{name}\s+\(?(-?\d+)\)?', open(HEADER).read()).group(1))


def test_library_exports_what_lt_expect_h_declares():
  """include/lt_expect.h declares the two entry points, the library exports
  them, the binding lists them, and lt_lattice.h pulls the header in."""
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(os.path.dirname(HEADER), 'lt_expect.h')).read(),
               flags=re.S)
  declared = sorted(set(re.findall(r'\b(lt_[a-z_]+)\s*\(', src)))
  assert declared == sorted(_native.EXPORTED_EXPECT) and len(declared) == 2
  for name in declared:
    assert hasattr(_native.lib(), name) and name in _native._SIG
  assert '#include "lt_expect.h"' in open(HEADER).read()


def test_expectation_host_validation_error_codes():
  lib = _native.lib()
  EINVAL, EUNSUPPORTED = _define('LT_EINVAL'), _define('LT_EUNSUPPORTED')
  null = ctypes.c_void_p(0)
  # host arrays stand in for the device pointers: nothing below dereferences them
  buf = (ctypes.c_int64 * 64)()
  p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)

  def graph(**kw):
    return dummy_graph(p, **kw)

  TP = _native.TableProblem
  ok = TP(batch=2, max_frames=4, max_labels=0, weight_dtype=0)
  nbytes = ctypes.c_size_t(7)

  def query(g, pb):
    return lib.lt_table_expectation_workspace_bytes(ctypes.byref(g), ctypes.byref(pb),
                                                    ctypes.byref(nbytes))

  assert query(graph(), ok) == 0
  need = nbytes.value
  assert need >= 2 * 4 * 2 * 4 * 33  # the alpha and mean histories, [B,T,C] fp32 each

  def call(g, pb, W=p, v=p, nf=p, E=p, lz=p, marg=p, cov=p, ws=p, n=None):
    return lib.lt_table_expectation(ctypes.byref(g), ctypes.byref(pb), W, v, nf, E, lz, marg, cov,
                                    ws, need if n is None else n, null)

  assert lib.lt_table_expectation(None, ctypes.byref(ok), p, p, p, p, p, p, p, p, need,
                                  null) == EINVAL
  assert call(graph(), ok, E=null) == EINVAL
  assert b'null output' in lib.lt_last_error()
  assert call(graph(), ok, lz=null) == EINVAL
  assert call(graph(), ok, W=null) == EINVAL
  assert call(graph(), ok, v=null) == EINVAL
  assert call(graph(), ok, nf=null) == EINVAL
  assert call(graph(), ok, ws=null) == EINVAL
  assert call(graph(), ok, n=need - 1) == EINVAL
  assert b'workspace' in lib.lt_last_error()
  assert call(graph(), TP(batch=2, max_frames=4, max_labels=0, weight_dtype=5)) == EINVAL
  assert call(graph(), TP(batch=-1, max_frames=4, max_labels=0, weight_dtype=0)) == EINVAL
  assert call(graph(), TP(batch=2, max_frames=-4, max_labels=0, weight_dtype=0)) == EINVAL
  assert call(graph(K=1), ok) == EUNSUPPORTED
  assert query(graph(K=2), ok) == EUNSUPPORTED
  # 8 vectors of C floats past 160 KiB of LDS
  assert query(graph(C=6000, V=2), ok) == EUNSUPPORTED
  assert b'LDS' in lib.lt_last_error()
  assert call(graph(C=6000, V=2), ok) == EUNSUPPORTED
  # an empty batch launches nothing and needs no inputs
  assert call(graph(), TP(batch=0, max_frames=4, max_labels=0, weight_dtype=0), W=null, v=null,
              nf=null, ws=null, n=0) == 0
  bench = TP(batch=64, max_frames=1000, max_labels=0, weight_dtype=1)
  assert query(graph(), bench) == 0
  assert nbytes.value >= 2 * 4 * 64 * 1000 * 33
