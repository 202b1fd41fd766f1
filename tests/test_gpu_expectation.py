"""RecognitionLattice.expectation on the GPU (lt_table_expectation,
lt_expect.hip) against cpu.expectation in float64 on the same inputs (and,
for one case, against the enumeration of every path directly).

W = randn - 2, so log alpha drifts by tens over an utterance and the integer
shift is exercised; num_frames = [T, T-3, 1, 0]. Tolerances:
* log_z and E: rtol = atol = 1e-4, the project's Log parity bound.
* marg: rtol 1e-4, atol 1e-5 max(1, max |ref|), as in test_gpu_table_grad.py.
* cov is a difference of path-length sums whose fp32 error nobody has
  measured, so it is held against a measured yardstick: per case, e32 = the
  largest error of cpu.expectation run in float32 against the float64
  reference; the kernel gets 4 e32 (both are fp32 evaluations of the same
  recurrences in different summation orders; 4x covers the order and the
  hardware exp), and is never held tighter than marg's bound. Both errors are
  printed per case (pytest -s; the table is kept in profiles/expect_parity.txt).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import last_torch_amd as lt
from last_torch_amd import _native
import expect_ref as ref

pytestmark = pytest.mark.gpu
B = 4


def _nf(T):
  return [T, T - 3, 1, 0]


def _context(name):
  rng = np.random.default_rng(5)
  if name == 'enum_v2_t5':
    return lt.contexts.FullNGram(vocab_size=2, context_size=1), 5
  if name in ('bigram_v32', 'bigram_v32_bf16'):
    return lt.contexts.FullNGram(vocab_size=32, context_size=1), 41
  if name == 'trigram_v5':
    return lt.contexts.FullNGram(vocab_size=5, context_size=2), 20
  if name == 'table_c17_v6':
    return lt.contexts.NextStateTable(ref.random_table(rng, 17, 6)), 30
  if name == 'table_c40_v6_two_sinks':  # in-degree 120: several passes of a G-lane group
    sinks = ((0, 5), (1, 5), (2, 5), (3, 11), (4, 11))
    return lt.contexts.NextStateTable(ref.random_table(rng, 40, 6, sinks)), 12
  if name == 'table_c300_v28':  # a 35 KB frame: the unstaged variant
    return lt.contexts.NextStateTable(ref.random_table(rng, 300, 28)), 8
  if name == 'masked_v6':
    return lt.contexts.FullNGram(vocab_size=6, context_size=1), 12
  raise KeyError(name)


CASES = ['enum_v2_t5', 'bigram_v32', 'bigram_v32_bf16', 'trigram_v5', 'table_c17_v6',
         'table_c40_v6_two_sinks', 'table_c300_v28', 'masked_v6']


def _table_of(context):
  if isinstance(context, lt.contexts.NextStateTable):
    return torch.as_tensor(context.next_state_table)
  return torch.as_tensor(context.next_state_table())


@functools.lru_cache(maxsize=None)
def _case(name):
  """Inputs (host tensors) and the float64 / float32 CPU references, once."""
  context, T = _context(name)
  C, V = _table_of(context).shape
  g = torch.Generator().manual_seed(CASES.index(name))
  nb = B + 1 if name == 'masked_v6' else B
  W = torch.randn([nb, T, C, V + 1], generator=g) - 2
  v = torch.randn([nb, T, C, V + 1], generator=g)
  nf = _nf(T)
  if name == 'masked_v6':
    off = torch.rand([nb, T, C, V + 1], generator=g) < 0.3
    W[off] = -torch.inf
    v[off] = torch.nan          # never read into the arithmetic
    W[4, 0, 0, :] = -torch.inf  # nothing leaves the start state: no path at all
    nf = nf + [T]
  if name.endswith('bf16'):
    W = W.bfloat16()
  if name == 'enum_v2_t5':  # the enumeration itself is the reference
    Wd = W.double().requires_grad_(True)
    vd = v.double().requires_grad_(True)
    E, log_z, _ = ref.enumerate_bigram(Wd, vd, nf)
    dW, dv = ref.grads(E, log_z, [Wd, vd], b=torch.zeros(nb))
    r64 = {k: x.detach().numpy() for k, x in (('E', E), ('log_z', log_z), ('dW', dW), ('dv', dv))}
  else:
    r64 = ref.cpu_reference(W.float(), v, nf, context, b=torch.zeros(nb))
  r32 = ref.cpu_reference(W.float(), v, nf, context, b=torch.zeros(nb), dtype=torch.float32)
  out = dict(context=context, T=T, W=W, v=v, nf=nf, E=r64['E'], log_z=r64['log_z'],
             cov=r64['dW'], marg=r64['dv'])
  out['marg_atol'] = 1e-5 * max(1.0, float(np.abs(out['marg']).max()))
  out['e32'] = float(np.abs(r32['dW'] - out['cov']).max())
  return out


def _marg_bound(c, scale=1.0):
  return scale * (c['marg_atol'] + 1e-4 * np.abs(c['marg']))


def _cov_bound(c):
  return np.maximum(4 * c['e32'], c['marg_atol'] + 1e-4 * np.abs(c['cov']))


def _native_call(c, cuda, want_marg=True, want_cov=True):
  lat = ref.table_lattice(c['context'], c['W'])
  graph = lat._graph(cuda)
  nf = torch.tensor(c['nf'], dtype=torch.int32, device=cuda)
  out = _native.table_expectation(graph, c['W'].to(cuda).contiguous(), c['v'].to(cuda), nf,
                                  want_marg, want_cov)
  torch.cuda.synchronize()
  return out


@pytest.mark.parametrize('name', CASES)
def test_parity(cuda, name):
  c = _case(name)
  E, log_z, marg, cov = (x.double().cpu().numpy() for x in _native_call(c, cuda))
  for x in (E, marg, cov):
    assert np.isfinite(x).all()
  assert not np.isnan(log_z).any()
  em = float(np.abs(marg - c['marg']).max())
  ec = float(np.abs(cov - c['cov']).max())
  fin = np.isfinite(c['log_z'])
  print(f"\nexpect_parity {name}: |E| {np.abs(E - c['E']).max():.3g} "
        f"|log_z| {np.abs(log_z[fin] - c['log_z'][fin]).max():.3g} "
        f"marg {em:.3g} (atol {c['marg_atol']:.3g}) cov: cpu fp32 {c['e32']:.3g} "
        f"kernel {ec:.3g} bound {max(4 * c['e32'], c['marg_atol']):.3g} "
        f"max|cov| {np.abs(c['cov']).max():.3g}")
  np.testing.assert_allclose(log_z, c['log_z'], rtol=1e-4, atol=1e-4)
  np.testing.assert_allclose(E, c['E'], rtol=1e-4, atol=1e-4)
  assert (np.abs(marg - c['marg']) <= _marg_bound(c)).all()
  assert (np.abs(cov - c['cov']) <= _cov_bound(c)).all()
  nf = c['nf']
  assert E[3] == 0 and log_z[3] == 0 and not marg[3].any() and not cov[3].any()  # nf = 0
  assert not marg[1, nf[1]:].any() and not cov[1, nf[1]:].any()                   # padding
  if name == 'masked_v6':
    off = ~np.isfinite(c['W'].float().numpy())
    assert not marg[off].any() and not cov[off].any()
    assert log_z[4] == -np.inf and E[4] == 0 and not marg[4].any() and not cov[4].any()


@pytest.mark.parametrize('name', ['bigram_v32', 'bigram_v32_bf16', 'table_c40_v6_two_sinks',
                                  'table_c300_v28'])
def test_marg_matches_the_den_backward_kernel(cuda, name):
  """marg is the quantity lt_table_den_backward (Log) writes: equal within
  that kernel's own parity bound."""
  c = _case(name)
  _, log_z, marg, _ = _native_call(c, cuda, want_cov=False)
  lat = ref.table_lattice(c['context'], c['W'])
  graph = lat._graph(cuda)
  W = c['W'].to(cuda).contiguous()
  nf = torch.tensor(c['nf'], dtype=torch.int32, device=cuda)
  dist, alpha = _native.table_forward(graph, W, nf, _native.SEMIRING_LOG)
  want = _native.table_den_backward(graph, W, nf, _native.SEMIRING_LOG, dist, alpha)
  np.testing.assert_allclose(log_z.cpu().numpy(), dist.cpu().numpy(), rtol=1e-4, atol=1e-4)
  want = want.double().cpu().numpy()
  bound = c['marg_atol'] + 1e-4 * np.abs(want)
  if name.endswith('bf16'):  # that kernel rounds its output to bf16
    bound = bound + 2.0 ** -8 * np.abs(want)
  assert (np.abs(marg.double().cpu().numpy() - want) <= bound).all()


def _public(c, cuda, w_grad, v_grad):
  table = c['W'].float().to(cuda).requires_grad_(w_grad)
  v = c['v'].to(cuda).requires_grad_(v_grad)
  lat = ref.table_lattice(c['context'], table)
  nf = torch.tensor(c['nf'], device=cuda)
  E, log_z = lat.expectation(ref.frames([len(c['nf'])], c['T'], cuda), nf, v)
  return table, v, E, log_z


@pytest.mark.parametrize('which', ['both', 'w_only', 'values_only'])
def test_incoming_gradients(cuda, which, monkeypatch):
  c = _case('table_c17_v6')
  asked = []
  real = _native.table_expectation

  def spy(graph, W, values, nf, want_marg=True, want_cov=True):
    asked.append((want_marg, want_cov))
    return real(graph, W, values, nf, want_marg, want_cov)

  monkeypatch.setattr(_native, 'table_expectation', spy)
  g = torch.Generator().manual_seed(3)
  a, b = torch.randn([B], generator=g), torch.randn([B], generator=g)
  table, v, E, log_z = _public(c, cuda, which != 'values_only', which != 'w_only')
  assert E.device == cuda and log_z.device == cuda
  (a.to(cuda) * E + b.to(cuda) * log_z).sum().backward()
  assert asked == [(True, which != 'values_only')]
  an, bn = a.double().numpy()[:, None, None, None], b.double().numpy()[:, None, None, None]
  if which != 'values_only':
    want = an * c['cov'] + bn * c['marg']
    bound = np.abs(an) * _cov_bound(c) + np.abs(bn) * _marg_bound(c)
    assert (np.abs(table.grad.double().cpu().numpy() - want) <= bound).all()
  else:
    assert table.grad is None
  if which != 'w_only':
    assert (np.abs(v.grad.double().cpu().numpy() - an * c['marg']) <=
            np.abs(an) * _marg_bound(c)).all()
  else:
    assert v.grad is None


def test_second_backward_recomputes(cuda):
  c = _case('table_c17_v6')
  table, v, E, log_z = _public(c, cuda, True, True)
  loss = (E + 0.5 * log_z).sum()
  loss.backward(retain_graph=True)
  gw, gv = table.grad.clone(), v.grad.clone()
  table.grad = v.grad = None
  loss.backward()
  assert torch.equal(table.grad, gw) and torch.equal(v.grad, gv)


@pytest.mark.parametrize('name', ['bigram_v32', 'table_c300_v28'])
def test_two_calls_are_bit_equal(cuda, name):
  c = _case(name)
  first, second = _native_call(c, cuda), _native_call(c, cuda)
  for x, y in zip(first, second):
    assert torch.equal(x, y)


def test_value_only_call_matches(cuda):
  c = _case('bigram_v32')
  E, log_z, marg, cov = _native_call(c, cuda, want_marg=False, want_cov=False)
  assert marg is None and cov is None
  E2, log_z2, _, _ = _native_call(c, cuda)
  assert torch.equal(E, E2) and torch.equal(log_z, log_z2)


def test_batch_dims(cuda):
  c = _case('table_c17_v6')
  T, W, v = c['T'], c['W'], c['v']
  lat = ref.table_lattice(c['context'], W.reshape(2, 2, *W.shape[1:]).to(cuda))
  E, log_z = lat.expectation(ref.frames([2, 2], T, cuda), torch.tensor(c['nf']).reshape(2, 2),
                             v.reshape(2, 2, *v.shape[1:]))
  assert tuple(E.shape) == (2, 2) and tuple(log_z.shape) == (2, 2) and E.device == cuda
  np.testing.assert_allclose(E.reshape(-1).cpu().numpy(), c['E'], rtol=1e-4, atol=1e-4)
  np.testing.assert_allclose(log_z.reshape(-1).cpu().numpy(), c['log_z'], rtol=1e-4, atol=1e-4)


def test_differentiable_entropy(cuda):
  """entropy(differentiable=True) on bigram_v32: the value against entropy(),
  dH/dW (a cov, of the values -W) against the float64 CPU path under cov's
  rule."""
  c = _case('bigram_v32')
  W, nf, T = c['W'], c['nf'], c['T']
  r64 = ref.cpu_reference(W, -W, nf, c['context'])   # H = log_z + E[-w]
  r32 = ref.cpu_reference(W, -W, nf, c['context'], dtype=torch.float32)
  # d H / d W = (d E / d W + d log_z / d W) - d E / d values
  want = r64['dW'] - r64['dv']
  e32 = float(np.abs((r32['dW'] - r32['dv']) - want).max())
  table = W.to(cuda).requires_grad_(True)
  lat = ref.table_lattice(c['context'], table)
  H = lat.entropy(ref.frames([B], T, cuda), torch.tensor(nf, device=cuda), differentiable=True)
  H0 = lat.entropy(ref.frames([B], T, cuda), torch.tensor(nf, device=cuda))
  np.testing.assert_allclose(H.detach().cpu().numpy(), H0.cpu().numpy(), rtol=1e-4, atol=1e-4)
  np.testing.assert_allclose(H.detach().cpu().numpy(), r64['log_z'] + r64['E'], rtol=1e-4,
                             atol=1e-4)
  H.sum().backward()
  got = table.grad.double().cpu().numpy()
  err = float(np.abs(got - want).max())
  print(f'\nexpect_parity entropy dH/dW bigram_v32: cpu fp32 {e32:.3g} kernel {err:.3g}')
  assert (np.abs(got - want) <= np.maximum(4 * e32, c['marg_atol'] + 1e-4 * np.abs(want))).all()


def test_error_codes_on_the_device(cuda):
  c = _case('table_c17_v6')
  lat = ref.table_lattice(c['context'], c['W'])
  graph = lat._graph(cuda)
  W = c['W'].to(cuda).contiguous()
  v = c['v'].to(cuda)
  nf = torch.tensor(c['nf'], dtype=torch.int32, device=cuda)
  pb = _native._tproblem(graph, W)
  lib = _native.lib()
  nbytes = ctypes.c_size_t(0)
  assert lib.lt_table_expectation_workspace_bytes(ctypes.byref(graph.g), ctypes.byref(pb),
                                                  ctypes.byref(nbytes)) == 0
  ws = torch.empty([nbytes.value], dtype=torch.uint8, device=cuda)
  E = torch.full([B], 7.0, device=cuda)
  log_z = torch.full([B], 7.0, device=cuda)
  p = _native._ptr

  def call(g=graph.g, W=W, E=E, ws=ws, n=nbytes.value):
    return lib.lt_table_expectation(ctypes.byref(g), ctypes.byref(pb), p(W), p(v), p(nf), p(E),
                                    p(log_z), None, None, p(ws), n, _native._stream())

  fld = _native.Graph(graph.C, graph.V, 1, graph.table.data_ptr(), graph.in_off.data_ptr(),
                      graph.in_arc.data_ptr())
  assert call(g=fld) == _native.LT_EUNSUPPORTED
  assert call(n=nbytes.value - 1) == -1 and call(ws=None) == -1
  assert call(W=None) == -1 and call(E=None) == -1
  torch.cuda.synchronize()
  assert (E == 7).all() and (log_z == 7).all()  # nothing was launched
  assert call() == 0
  torch.cuda.synchronize()
  np.testing.assert_allclose(E.cpu().numpy(), c['E'], rtol=1e-4, atol=1e-4)
