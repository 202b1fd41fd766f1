"""The host twin's results do not depend on what its output buffers held.

Every output of ``_native_cpu`` comes from ``torch.empty`` / ``empty_like``,
usually zero pages the first time and the previous call's (correct) values
the second. Here each entry point runs once on 0xFF-poisoned allocations and
once on the tensors a finished call on ANOTHER problem of the same shape left
behind (tests/poisoned_buffers.py), on ragged batches (0, 1, T-1 and T frames;
an unreachable string, an empty one, epsilon labels), and EVERY element of
every output -- padding frames included -- is compared with the pinned C
oracle under the bounds of tests/test_cpu_twin.py.

The helper's own behaviour is tested at the top. CPU only.
"""
import types

import numpy as np
import pytest
import torch

from last_torch_amd import _native_cpu as cpu
from golden_cases import assert_grad_marginal_close, assert_loss_close, assert_values_close
from poisoned_buffers import poisoned, stale

LOG, MAX, REAL = 0, 1, 2


def _orc():
  from oracle import oracle as orc  # test infrastructure only
  return orc


# ---------------------------------------------------------------------------
# the helper itself
# ---------------------------------------------------------------------------
def _fake_module():
  """A stand-in for a binding module: reaches the allocator through its
  `torch` attribute only."""
  m = types.ModuleType('fake_binding')
  m.torch = torch

  def alloc(n=3, dtype=torch.float32):
    a = m.torch.empty([n, 2], dtype=dtype)
    b = m.torch.empty_like(a)
    c = m.torch.empty([n], dtype=torch.uint8)
    return a, b, c

  m.alloc = alloc
  return m


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.int32, torch.int64,
                                   torch.uint8])
def test_poisoned_fills_every_dtype(dtype):
  m = _fake_module()
  with poisoned(m):
    a, b, _ = m.alloc(5, dtype)
    z = m.torch.zeros([2])  # everything else is the real torch
    e = m.torch.empty([0], dtype=dtype)
  assert m.torch is torch and float(z.sum()) == 0 and e.numel() == 0
  for t in (a, b):
    assert t.dtype == dtype and t.shape == (5, 2)
    assert (t.reshape(-1).view(torch.uint8) == 0xFF).all()
    if dtype.is_floating_point:
      assert torch.isnan(t).all()
    elif dtype == torch.uint8:
      assert (t == 255).all()
    else:
      assert (t == -1).all()


def test_stale_replay_returns_the_identical_storages():
  m = _fake_module()
  with stale(m) as s:
    first = s.record(m.alloc)
    for i, t in enumerate(first):
      t.fill_(i + 1)
    second = s.replay(m.alloc)
    assert len(second) == len(first) == len(s.tensors)
    for i, (x, y) in enumerate(zip(first, second)):
      assert x is y and x.data_ptr() == y.data_ptr()
      assert (y == i + 1).all()  # as the first call left it
  assert m.torch is torch


def test_stale_replay_raises_on_mismatch():
  m = _fake_module()
  with stale(m) as s:
    s.record(m.alloc, 3)
    with pytest.raises(AssertionError, match='asks for'):
      s.replay(m.alloc, 4)  # another shape
    assert m.torch is torch
    with pytest.raises(AssertionError, match='asks for'):
      s.replay(m.alloc, 3, torch.int32)  # another dtype
    with pytest.raises(AssertionError, match='recorded'):
      s.replay(lambda: m.alloc(3) + (m.torch.empty([1]),))  # one allocation more
    with pytest.raises(AssertionError, match='recorded'):
      s.replay(lambda: m.torch.empty([3, 2]))  # fewer


# ---------------------------------------------------------------------------
# the twin on poisoned and stale buffers
# ---------------------------------------------------------------------------
B, T, U = 6, 37, 6
SHAPES = [(4, 0, torch.float32), (6, 1, torch.float32), (5, 2, torch.float32),
          (3, 3, torch.float32), (6, 1, torch.bfloat16), (4, 2, torch.bfloat16)]
NF = np.array([0, 1, T - 1, T, 2, T], np.int32)
NL = np.array([0, 1, U, 0, 5, U - 1], np.int32)  # utterance 4: 5 labels in 2 frames


def _problem(V, n, dtype, seed):
  """Ragged batch: 0, 1, T-1 and T frames; an unreachable string (utterance
  4), empty strings, epsilon (0) labels. `seed` also permutes the lengths, so
  that problems A and B differ in seeds, lengths and labels."""
  orc = _orc()
  rng = np.random.default_rng(seed)
  C = orc.num_states(V, n)
  W = rng.standard_normal((B, T, C, V + 1)).astype(np.float32)
  if dtype == torch.bfloat16:
    W = torch.tensor(W).bfloat16().float().numpy()
  perm = rng.permutation(B)
  lab = rng.integers(0, V + 1, (B, U)).astype(np.int32)
  lab[4] = rng.integers(1, V + 1, U)
  return W, NF[perm].copy(), lab[perm].copy(), NL[perm].copy()


def _host(p, dtype):
  W, nf, lab, nl = p
  return torch.tensor(W).to(dtype), torch.tensor(nf), torch.tensor(lab), torch.tensor(nl)


def _run(mode, fn, pa, pb):
  """fn(problem) under `mode` on problem B; in the stale mode after a finished
  call on problem A whose buffers B's call inherits."""
  if mode == 'poisoned':
    with poisoned(cpu):
      return fn(pb)
  with stale(cpu) as s:
    s.record(fn, pa)
    return s.replay(fn, pb)


MODES = ['poisoned', 'stale']


@pytest.fixture(scope='module')
def problems():
  """(A, B, B's oracle results) per shape, computed once."""
  cache = {}

  def get(V, n, dtype):
    key = (V, n, dtype)
    if key not in cache:
      orc = _orc()
      pa, pb = _problem(V, n, dtype, 300 + 10 * V + n), _problem(V, n, dtype, 900 + 10 * V + n)
      W, nf, lab, nl = pb
      assert not np.array_equal(pa[1], nf) or not np.array_equal(pa[2], lab)
      ref = {'loss': orc.loss_grad(W, nf, lab, nl, V, n),
             'loss_local': orc.loss_grad(W, nf, lab, nl, V, n, local_norm=True),
             'den_grad': orc.den_grad(W, nf, V, n)}
      for s in (LOG, MAX, REAL):
        ref['den', s] = orc.den_forward(W, nf, V, n, s)
        ref['num', s] = orc.num_forward(W, nf, lab, nl, V, n, s)
      for conv in (0, 1):
        ref['vit', conv] = orc.viterbi(W, nf, V, n, convention=conv, want_arcs=True)
      # the batch is what it claims: an unreachable string, an empty utterance
      assert np.isposinf(ref['loss'][0][nl > nf]).all() and (nl > nf).any()
      for v in ref.values():
        for x in v:
          x.setflags(write=False)
      cache[key] = (pa, pb, ref)
    return cache[key]

  return get


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('V,n,dtype', SHAPES)
def test_loss_grad(problems, V, n, dtype, mode):
  """lt_cpu_loss_grad, global and local normalisation: loss, log_z, num and
  every dW element (0 on padding frames and for the unreachable string)."""
  pa, pb, ref = problems(V, n, dtype)
  bf16 = dtype == torch.bfloat16
  for local in (False, True):
    loss, lz, num, dW = _run(mode, lambda p: cpu.loss_grad(*_host(p, dtype), V, n, local), pa, pb)
    rl, rlz, rnum, rdW = ref['loss_local' if local else 'loss']
    assert_loss_close(loss.numpy(), rl)
    assert_loss_close(num.numpy(), rnum)
    if local:  # no denominator: log_z = 0, exactly
      np.testing.assert_array_equal(lz.numpy(), np.zeros_like(rl))
    else:
      assert_loss_close(lz.numpy(), rlz)
    assert_grad_marginal_close(dW.float().numpy(), rdW, None if local else ref['den_grad'][1],
                               rlz, rnum, bf16)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('V,n,dtype', SHAPES)
def test_den_forward_and_backward(problems, V, n, dtype, mode):
  """lt_cpu_den_forward in the three semirings (alpha with its carried
  padding rows) and lt_cpu_den_backward."""
  pa, pb, ref = problems(V, n, dtype)
  bf16 = dtype == torch.bfloat16
  for s in (LOG, MAX, REAL):
    d, a = _run(mode, lambda p: cpu.den_forward(*_host(p, dtype)[:2], V, n, s), pa, pb)
    rd, ra = ref['den', s]
    if s == MAX:
      np.testing.assert_array_equal(d.numpy(), rd)
      np.testing.assert_array_equal(a.numpy(), ra)
    elif s == LOG:
      assert_loss_close(d.numpy(), rd)
      assert_values_close(a.numpy(), ra, rtol=1e-4, atol=1e-4)
    else:
      scale = max(1.0, float(np.abs(rd).max()))
      assert_values_close(d.numpy(), rd, rtol=1e-4, atol=1e-5 * scale)
      ascale = max(1.0, float(np.abs(ra).max()))  # partial distances: the distance's bound
      assert_values_close(a.numpy(), ra, rtol=1e-4, atol=1e-5 * ascale)

  def bwd(p):
    W, nf = _host(p, dtype)[:2]
    lz, al = cpu.den_forward(W, nf, V, n, LOG)
    return cpu.den_backward(W, nf, lz, al, V, n)

  dW = _run(mode, bwd, pa, pb)
  rlz, den = ref['den_grad']
  assert_grad_marginal_close(dW.float().numpy(), den, den, rlz, None, bf16)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('V,n,dtype', SHAPES)
def test_num_forward(problems, V, n, dtype, mode):
  """lt_cpu_num_forward in the three semirings: num and the whole alpha_num
  history, padding rows included."""
  pa, pb, ref = problems(V, n, dtype)
  for s in (LOG, MAX, REAL):
    num, an = _run(mode, lambda p: cpu.num_forward(*_host(p, dtype), V, n, s), pa, pb)
    rn, ran = ref['num', s]
    if s == MAX:
      np.testing.assert_array_equal(num.numpy(), rn)
      np.testing.assert_array_equal(an.numpy(), ran)
    elif s == LOG:
      assert_loss_close(num.numpy(), rn)
      assert_values_close(an.numpy(), ran, rtol=1e-4, atol=1e-4)
    else:
      scale = max(1.0, float(np.abs(rn).max()))
      assert_values_close(num.numpy(), rn, rtol=1e-4, atol=1e-5 * scale)
      ascale = max(1.0, float(np.abs(ran).max()))  # partial distances: the distance's bound
      assert_values_close(an.numpy(), ran, rtol=1e-4, atol=1e-5 * ascale)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('V,n,dtype', SHAPES)
def test_viterbi(problems, V, n, dtype, mode):
  """lt_cpu_viterbi, both label conventions: labels (0 on padding frames),
  path weights and the one-hot arcs, bit-exact."""
  pa, pb, ref = problems(V, n, dtype)
  for conv in (0, 1):
    labels, wts, arcs = _run(
        mode, lambda p: cpu.viterbi(*_host(p, dtype)[:2], V, n, conv, with_arcs=True), pa, pb)
    rlab, rw, rarcs = ref['vit', conv]
    np.testing.assert_array_equal(labels.numpy(), rlab)
    np.testing.assert_array_equal(wts.numpy(), rw)
    np.testing.assert_array_equal(arcs.float().numpy(), rarcs)
