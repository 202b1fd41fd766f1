"""Kernel results do not depend on what their output buffers and workspaces
held before the call.

Every output and workspace of ``_native`` comes from ``torch.empty`` /
``empty_like``: zero pages on a first allocation, the previous call's own
(correct) values on the rerun the determinism checks make. Here every entry
point of the C ABI runs

  * ``poisoned``: on allocations filled with 0xFF bytes (NaN / -1), and
  * ``stale``: on the very tensors -- outputs and workspaces -- that a finished
    call on ANOTHER problem of the same shape (other seed, lengths, labels)
    left behind, flags, tags and values included (tests/poisoned_buffers.py),

on ragged batches (0, 1, T-1 and T frames; an unreachable string, an empty
one, epsilon labels), and EVERY element of every output the headers define --
padding frames included -- is compared with the oracle and under the bound the
entry point's own parity test uses (test_gpu_parity.py, test_gpu_table.py,
test_gpu_table_grad.py, test_gpu_string_grad.py, test_gpu_align.py,
test_gpu_sample.py, test_gpu_expectation.py, test_gpu_producer.py,
test_gpu_joint_fused.py). No tolerance is new.

The fused pipe's granule tags are ``epoch * T + t`` with a per-process epoch,
so its stale-tag case runs in a child process (pipe_stale_child.py).

lt_scale_grad writes in place and allocates nothing: it has no case here.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from last_torch_amd import _native as nat
from golden_cases import (assert_grad_marginal_close, assert_loss_close, assert_values_close,
                          table_den_marginals)
from poisoned_buffers import poisoned, stale
import align_compact
import expect_ref
import sample_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ['poisoned', 'stale']
LOG, MAX, REAL = nat.SEMIRING_LOG, nat.SEMIRING_MAX, nat.SEMIRING_REAL


def _orc():
  from oracle import oracle as orc  # test infrastructure only
  return orc


def _run(mode, fn, a, b):
  """fn(b) under `mode`; in the stale mode after a finished fn(a), whose
  allocations (outputs and workspaces, as that call left them) fn(b) gets."""
  if mode == 'poisoned':
    with poisoned(nat):
      out = fn(b)
  else:
    with stale(nat) as s:
      s.record(fn, a)
      torch.cuda.synchronize()
      out = s.replay(fn, b)
  torch.cuda.synchronize()
  return out


_CACHE = {}


def _cached(key, make):
  """Problems and their oracle results, computed once and shared (read-only)
  among the modes and designs."""
  if key not in _CACHE:
    _CACHE[key] = make()
  return _CACHE[key]


def _freeze(ref):
  for v in ref.values():
    for x in (v if isinstance(v, tuple) else (v,)):
      if isinstance(x, np.ndarray):
        x.setflags(write=False)
  return ref


def _lengths(B, T, U, per=1):
  """Ragged lengths of B >= 6 utterances: T, 0, 1 and T-1 frames; utterance 4
  has more labels than its 2 frames can emit (`per` lexical arcs a frame at
  the most), utterance 5 an empty string."""
  assert 6 <= B <= 8 and U >= 2 * per + 1
  nf = np.array([T, 0, 1, T - 1, 2, T, T // 2, T - 2], np.int32)[:B]
  nl = np.array([min(U, T * per), 0, 1, min(U, (T - 1) * per), 2 * per + 1, 0,
                 min(U, T // 2) // 2, 1], np.int32)[:B]
  return nf, nl


def _ngram_problem(B, T, U, V, n, bf16, seed, lengths=None):
  """(W, nf, lab, nl) as numpy: ragged (see _lengths, or `lengths`), labels
  with epsilons; `seed` also permutes the lengths among the utterances, so two
  seeds differ in weights, lengths and labels."""
  orc = _orc()
  rng = np.random.default_rng(seed)
  C = orc.num_states(V, n)
  W = rng.standard_normal((B, T, C, V + 1)).astype(np.float32)
  if bf16:
    W = torch.tensor(W).bfloat16().float().numpy()
  nf, nl = lengths if lengths is not None else _lengths(B, T, U)
  perm = rng.permutation(B)
  lab = rng.integers(0, V + 1, (B, U)).astype(np.int32)
  return W, np.asarray(nf, np.int32)[perm].copy(), lab, np.asarray(nl, np.int32)[perm].copy()


def _dev(p, cuda, bf16):
  W, nf, lab, nl = p
  return (torch.tensor(W).to(torch.bfloat16 if bf16 else torch.float32).to(cuda),
          torch.tensor(nf).to(cuda), torch.tensor(lab).to(cuda), torch.tensor(nl).to(cuda))


def _real_weights(W, V, bf16, frames=12):
  """Positive weights whose products stay inside fp32 over `frames` frames
  (as test_gpu_string_grad.py's Real cases)."""
  Wr = (np.exp(W[:, :frames] - np.log(V + 1.0)) * 1.3).astype(np.float32)
  if bf16:
    Wr = torch.tensor(Wr).bfloat16().float().numpy()
  return Wr


def _assert_real_close(got, ref):
  """Real distances: test_gpu_parity.py's bound."""
  scale = max(1.0, float(np.abs(ref).max()))
  assert_values_close(got, ref, rtol=1e-4, atol=1e-5 * scale)


def _assert_real_grad_close(got, ref, bf16):
  """test_gpu_string_grad.py's bounds: rtol 1e-4 plus 1e-5 of each
  utterance's largest |element|; a bf16 dW 2^-8 relative."""
  got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
  assert np.isfinite(ref).all() and np.isfinite(got).all()
  if bf16:
    np.testing.assert_allclose(got, ref, rtol=2 ** -8 + 1e-4, atol=1e-30)
    return
  scale = np.abs(ref).reshape(ref.shape[0], -1).max(-1)
  tol = 1e-4 * np.abs(ref) + 1e-5 * scale.reshape(-1, *([1] * (ref.ndim - 1))) + 1e-30
  bad = np.abs(got - ref) > tol
  assert not bad.any(), (int(bad.sum()), float((np.abs(got - ref) / tol).max()))


def _np(t):
  return t.float().cpu().numpy()


# ---------------------------------------------------------------------------
# lt_den_forward, lt_den_backward, lt_num_forward
# ---------------------------------------------------------------------------
def _forward_case(V, n, bf16):
  def make():
    orc = _orc()
    B, T, U = 6, 24, 8
    pa = _ngram_problem(B, T, U, V, n, bf16, 1000 + 10 * V + n)
    pb = _ngram_problem(B, T, U, V, n, bf16, 2000 + 10 * V + n)
    W, nf, lab, nl = pb
    ref = {'den_grad': orc.den_grad(W, nf, V, n)}
    for s in (LOG, MAX):
      ref['den', s] = orc.den_forward(W, nf, V, n, s)
      ref['num', s] = orc.num_forward(W, nf, lab, nl, V, n, s)
    ra, rb = ((_real_weights(p[0], V, bf16, T),) + p[1:] for p in (pa, pb))
    ref['den', REAL] = orc.den_forward(rb[0], nf, V, n, REAL)
    ref['num', REAL] = orc.num_forward(rb[0], nf, lab, nl, V, n, REAL)
    return pa, pb, ra, rb, _freeze(ref)
  return _cached(('fwd', V, n, bf16), make)


FORWARD_SHAPES = [(32, 1), (8, 2), (32, 0)]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('V,n', FORWARD_SHAPES)
def test_den_forward_and_backward(cuda, V, n, dt, mode):
  """dist and the whole alpha history (padding rows carry alpha) in Log,
  MaxTropical and Real; d log_z / dW with its zeros on padding frames."""
  bf16 = dt == 'bf16'
  pa, pb, ra, rb, ref = _forward_case(V, n, bf16)
  for s in (LOG, MAX, REAL):
    a, b = ((ra, rb) if s == REAL else (pa, pb))
    da, db = _dev(a, cuda, bf16), _dev(b, cuda, bf16)
    d, al = _run(mode, lambda p: nat.den_forward(p[0], p[1], V, n, s), da, db)
    rd, ral = ref['den', s]
    if s == MAX:
      np.testing.assert_array_equal(_np(d), rd)
      np.testing.assert_array_equal(_np(al), ral)
    elif s == LOG:
      assert_loss_close(_np(d), rd)
      assert_values_close(_np(al), ral, rtol=1e-4, atol=1e-4)
    else:
      _assert_real_close(_np(d), rd)
      _assert_real_close(_np(al), ral)  # partial distances: the distance's own bound

  def bwd(p):
    lz, al = nat.den_forward(p[0], p[1], V, n, LOG)
    return nat.den_backward(p[0], p[1], lz, al, None, V, n)

  dW = _run(mode, bwd, _dev(pa, cuda, bf16), _dev(pb, cuda, bf16))
  rlz, den = ref['den_grad']
  assert_grad_marginal_close(_np(dW), den, den, rlz, None, bf16)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('V,n', FORWARD_SHAPES)
def test_num_forward(cuda, V, n, dt, mode):
  """num and the whole alpha_num history in Log and MaxTropical, num in Real."""
  bf16 = dt == 'bf16'
  pa, pb, ra, rb, ref = _forward_case(V, n, bf16)
  for s in (LOG, MAX, REAL):
    a, b = ((ra, rb) if s == REAL else (pa, pb))
    da, db = _dev(a, cuda, bf16), _dev(b, cuda, bf16)
    num, an = _run(mode, lambda p: nat.num_forward(*p, V, n, s), da, db)
    rn, ran = ref['num', s]
    if s == MAX:
      np.testing.assert_array_equal(_np(num), rn)
      np.testing.assert_array_equal(_np(an), ran)
    elif s == LOG:
      assert_loss_close(_np(num), rn)
      assert_values_close(_np(an), ran, rtol=1e-4, atol=1e-4)
    else:
      _assert_real_close(_np(num), rn)
      _assert_real_close(_np(an), ran)  # partial distances: the distance's own bound


# ---------------------------------------------------------------------------
# lt_loss_forward + lt_loss_backward, lt_loss_grad, lt_chunk_forward / backward
# ---------------------------------------------------------------------------
def _loss_case(name, B, T, U, V, n, bf16, lengths=None):
  def make():
    orc = _orc()
    la = lb = None
    if lengths is not None:
      la = lb = lengths
    pa = _ngram_problem(B, T, U, V, n, bf16, 31 + sum(map(ord, name)), la)
    pb = _ngram_problem(B, T, U, V, n, bf16, 77 + sum(map(ord, name)), lb)
    W, nf, lab, nl = pb
    ref = {False: orc.loss_grad(W, nf, lab, nl, V, n),
           True: orc.loss_grad(W, nf, lab, nl, V, n, local_norm=True),
           'den': orc.den_grad(W, nf, V, n)[1]}
    # the batch is what it claims: its over-long strings are unreachable
    assert (nl > nf).any() and np.isposinf(ref[False][0][nl > nf]).all()
    assert not np.array_equal(pa[1], nf) or not np.array_equal(pa[3], nl)
    return pa, pb, _freeze(ref)
  return _cached(('loss', name, bf16), make)


def _check_loss(out, ref, local, bf16):
  loss, lz, num, dW = out
  rl, rlz, rnum, rdW = ref[local]
  assert_loss_close(_np(loss), rl)
  assert_loss_close(_np(num), rnum)
  if local:  # no denominator: the header's log_z = 0, exactly
    np.testing.assert_array_equal(_np(lz), np.zeros_like(rl))
  else:
    assert_loss_close(_np(lz), rlz)
  assert_grad_marginal_close(_np(dW), rdW, None if local else ref['den'], rlz, rnum, bf16)


# the shape of test_gpu_parity.test_trigram_v32_short_and_empty_utterances,
# with one string (3 labels in 2 frames) made unreachable
TRIGRAM = dict(B=5, T=24, U=6, V=32, n=2,
               lengths=(np.array([24, 0, 1, 2, 23]), np.array([6, 0, 1, 3, 5])))
BIGRAM = dict(B=8, T=24, U=12, V=32, n=1)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('local', [False, True])
@pytest.mark.parametrize('ckpt', [False, True])
@pytest.mark.parametrize('name', ['bigram', 'trigram_bf16'])
def test_loss_forward_backward(cuda, name, ckpt, local, mode):
  """loss, log_z, num, the whole alpha and alpha_num histories and every dW
  element; the checkpoints (beta, beta_num, arcs) are the pair's internal
  hand-off, checked through dW."""
  bf16 = name == 'trigram_bf16'
  shape = TRIGRAM if bf16 else BIGRAM
  pa, pb, ref = _loss_case(name, bf16=bf16, **shape)
  V, n = shape['V'], shape['n']

  def fn(p):
    out = nat.loss_forward(*p, V, n, local, checkpoints=ckpt)
    dW = nat.loss_backward(*p, *out[1:5], None, V, n, local, ck=out[5] if ckpt else None)
    return out[0], out[1], out[2], dW, out[3], out[4]

  out = _run(mode, fn, _dev(pa, cuda, bf16), _dev(pb, cuda, bf16))
  _check_loss(out[:4], ref, local, bf16)
  # alpha and alpha_num are the den / num forward's histories, padding rows too
  W, nf, lab, nl = pb
  ral, ran = _cached(('loss_alpha', name), lambda: (
      _orc().den_forward(W, nf, V, n, LOG)[1], _orc().num_forward(W, nf, lab, nl, V, n, LOG)[1]))
  if local:
    assert out[4] is None  # no denominator, no alpha tensor
  else:
    assert_values_close(_np(out[4]), ral, rtol=1e-4, atol=1e-4)
  assert_values_close(_np(out[5]), ran, rtol=1e-4, atol=1e-4)


LOSS_GRAD_SHAPES = {
    # chunk lengths 7 and 6: three chunks each, the last of one frame
    'v32_u30_t15': dict(B=8, T=15, U=30, V=32, n=1),
    'v32_u100_t13': dict(B=8, T=13, U=100, V=32, n=1),
    'v16_u30_t15': dict(B=8, T=15, U=30, V=16, n=1),
}


def test_loss_grad_shapes_span_three_chunks():
  """The V = 32 shapes above are cut into chunks of 7 (U = 30) and 6 (U = 100)
  frames, the last chunk of one frame (bench.chunk_len mirrors ck_plan's LDS
  budget; test_gpu_chunk_geometry.py pins it)."""
  import bench
  for name, L in (('v32_u30_t15', 7), ('v32_u100_t13', 6)):
    c = LOSS_GRAD_SHAPES[name]
    assert bench.chunk_len(c['B'], c['T'], c['U'], c['V']) == L
    assert c['T'] == 2 * L + 1


DESIGNS = {'chunk': nat.DESIGN_CHUNK, 'fused_pipe': nat.DESIGN_FUSED_PIPE,
           'checkpoints': nat.DESIGN_CHECKPOINTS, 'recursion': nat.DESIGN_RECURSION}


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('design', list(DESIGNS))
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('name', list(LOSS_GRAD_SHAPES))
def test_loss_grad(cuda, name, dt, design, mode):
  """lt_loss_grad_ex in each design. The stale mode runs twice: once with the
  workspace from the allocator, once with one caller-owned workspace handed to
  both calls through ``workspace=``, after which the chunked design sent only
  the unreachable strings to the frame-serial kernels (their documented
  route) and no fused hand-off wait timed out."""
  bf16 = dt == 'bf16'
  shape = LOSS_GRAD_SHAPES[name]
  pa, pb, ref = _loss_case(name, bf16=bf16, **shape)
  B, U, V, n = shape['B'], shape['U'], shape['V'], shape['n']
  d = DESIGNS[design]
  da, db = _dev(pa, cuda, bf16), _dev(pb, cuda, bf16)
  for local in (False, True):
    out = _run(mode, lambda p: nat.loss_grad(*p, V, n, local, design=d), da, db)
    _check_loss(out, ref, local, bf16)
    if mode == 'stale':
      nb = nat.loss_grad_workspace_bytes(db[0], V, n, U, local, d)
      ws = torch.full([max(nb, 1)], 0xFF, dtype=torch.uint8, device=cuda)
      out = _run(mode, lambda p: nat.loss_grad(*p, V, n, local, workspace=ws, design=d), da, db)
      _check_loss(out, ref, local, bf16)
      if d == nat.DESIGN_CHUNK:
        # the state's per-utterance fallback words: an unreachable string is
        # the frame-serial kernels' by design (include/lt_lattice.h); no other
        # utterance may have left the chunked kernels
        fell = ws[:4 * B].view(torch.int32).ne(0).cpu().numpy()
        np.testing.assert_array_equal(fell, np.isneginf(ref[local][2]))
        assert nat.chunk_fallback_count(ws, B) == int(np.isneginf(ref[local][2]).sum())
      if d == nat.DESIGN_FUSED_PIPE:
        assert nat.grad_workspace_errors(ws, db[0], V, n, U, local) == 0


@pytest.mark.parametrize('mode', MODES)
def test_trigram_overlap_loss_grad(cuda, mode):
  """lt_loss_grad's trigram V = 32 route (tri_mix_kernel): the `done` words
  the marginal workgroups poll are cleared by a memset of a computed size."""
  B, T, U, V, n = 8, 160, 12, 32, 2
  lengths = (np.array([T, 0, 1, 2, T - 1, 150, 3, T]), np.array([U, 0, 1, 2, U - 1, U, 5, U]))
  pa, pb, ref = _loss_case('trigram_overlap', B, T, U, V, n, True, lengths)
  assert nat.loss_grad_design(B, T, U, V, n, True) == nat.DESIGN_CHECKPOINTS
  out = _run(mode, lambda p: nat.loss_grad(*p, V, n, False), _dev(pa, cuda, True),
             _dev(pb, cuda, True))
  _check_loss(out, ref, False, True)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('name', list(LOSS_GRAD_SHAPES))
def test_chunk_forward_backward(cuda, name, dt, mode):
  """lt_chunk_forward then lt_chunk_backward: `state` and both `scratch`
  buffers come from the allocator."""
  bf16 = dt == 'bf16'
  shape = LOSS_GRAD_SHAPES[name]
  pa, pb, ref = _loss_case(name, bf16=bf16, **shape)
  V, n = shape['V'], shape['n']
  for local in (False, True):

    def fn(p):
      loss, lz, num, state = nat.chunk_forward(*p, V, n, local)
      return loss, lz, num, nat.chunk_backward(*p, V, n, local, state)

    _check_loss(_run(mode, fn, _dev(pa, cuda, bf16), _dev(pb, cuda, bf16)), ref, local, bf16)


# ---------------------------------------------------------------------------
# lt_viterbi
# ---------------------------------------------------------------------------
VITERBI = {
    'bigram_v32': dict(B=6, T=40, V=32, n=1, bf16=False),
    'bigram_v32_bf16': dict(B=6, T=40, V=32, n=1, bf16=True),
    'trigram_v8': dict(B=6, T=40, V=8, n=2, bf16=False),
    # past the one-launch range (T <= 2,300 at V = 32): the backtrace is a
    # second launch that reads its backpointers from the workspace
    'bigram_v32_t2400': dict(B=2, T=2400, V=32, n=1, bf16=False, lengths=[2400, 1]),
}


def _viterbi_case(name):
  def make():
    orc = _orc()
    c = VITERBI[name]
    B, T, V, n = c['B'], c['T'], c['V'], c['n']
    out = []
    for seed in (5, 6):
      W, nf, _, _ = _ngram_problem(max(B, 6), T, 3, V, n, c['bf16'], seed + sum(map(ord, name)))
      W, nf = W[:B], nf[:B]
      if 'lengths' in c:
        nf = np.array(c['lengths'] if seed == 6 else c['lengths'][::-1], np.int32)
      out.append((np.ascontiguousarray(W), nf))
    W, nf = out[1]
    ref = {conv: orc.viterbi(W, nf, V, n, convention=conv, want_arcs=True) for conv in (0, 1)}
    return out[0], out[1], _freeze(ref)
  return _cached(('viterbi', name), make)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', list(VITERBI))
def test_viterbi(cuda, name, mode):
  """Labels (0 on padding frames), path weights and the one-hot arcs,
  bit-exact, in both label conventions."""
  c = VITERBI[name]
  pa, pb, ref = _viterbi_case(name)
  dt = torch.bfloat16 if c['bf16'] else torch.float32
  da, db = ((torch.tensor(W).to(dt).to(cuda), torch.tensor(nf).to(cuda)) for W, nf in (pa, pb))
  for conv in (nat.LABELS_TRUE, nat.LABELS_REFERENCE):
    labels, weights, arcs = _run(
        mode, lambda p: nat.viterbi(p[0], p[1], c['V'], c['n'], conv, want_arcs=True), da, db)
    rlab, rw, rarcs = ref[conv]
    np.testing.assert_array_equal(labels.cpu().numpy(), rlab)
    np.testing.assert_array_equal(_np(weights), rw)
    np.testing.assert_array_equal(_np(arcs), rarcs)


# ---------------------------------------------------------------------------
# the general table kernels (lt_table.hip)
# ---------------------------------------------------------------------------
def _table_problem(rng, tab, B, T, U, K, bf16):
  C, V = tab.shape
  W = rng.standard_normal((B, T, C, V + 1)).astype(np.float32)
  if bf16:
    W = torch.tensor(W).bfloat16().float().numpy()
  nf, nl = _lengths(B, T, U, max(K, 1))
  perm = rng.permutation(B)
  lab = rng.integers(0, V + 1, (B, U)).astype(np.int32)
  return W, nf[perm].copy(), lab, nl[perm].copy()


def _table_case(K, bf16):
  def make():
    orc = _orc()
    C, V, B, T, U = 7, 4, 6, 30, 6  # test_gpu_table.RANDOM_DFA's first rows, ragged
    rng = np.random.default_rng(C * 100 + V * 10 + K)
    tab = rng.integers(0, C, (C, V)).astype(np.int32)
    pa = _table_problem(rng, tab, B, T, U, K, bf16)
    pb = _table_problem(rng, tab, B, T, U, K, bf16)
    W, nf, lab, nl = pb
    ref = {'den': table_den_marginals(orc, tab, W, nf, lab, nl, K)}
    for s in (LOG, MAX):
      ref['fwd', s] = orc.tab_den_forward(tab, W, nf, K, s, want_alpha=True)
      ref['num', s] = orc.tab_num_forward(tab, W, nf, lab, nl, K, s)
    for local in (False, True):
      ref['loss', local] = orc.tab_loss_grad(tab, W, nf, lab, nl, K, local_norm=local)
    assert (nl > nf * max(K, 1)).any() and np.isposinf(ref['loss', False][0][nl > nf * max(K, 1)]).all()
    for conv in (0, 1):
      ref['vit', conv] = orc.tab_viterbi(tab, W, nf, K, conv)
    ref['den_grad', MAX] = orc.tab_dist_grad(tab, W, nf, K, orc.MAX)
    ref['num_grad', MAX] = orc.tab_dist_grad(tab, W, nf, K, orc.MAX, lab, nl)
    # Real: 12 frames of positive weights (test_gpu_string_grad.py)
    # with ragged lengths of their own (0, 1, 11 and 12 frames)
    ra, rb = ((_real_weights(p[0], V, bf16),) + _table_problem(rng, tab, B, 12, U, K, bf16)[1:]
              for p in (pa, pb))
    lab, nl = rb[2:]
    Wr, nfr = rb[:2]
    ref['fwd', REAL] = orc.tab_den_forward(tab, Wr, nfr, K, REAL, want_alpha=True)
    ref['num', REAL] = orc.tab_num_forward(tab, Wr, nfr, lab, nl, K, REAL)
    ref['den_grad', REAL] = orc.tab_dist_grad(tab, Wr, nfr, K, orc.REAL)
    ref['num_grad', REAL] = orc.tab_dist_grad(tab, Wr, nfr, K, orc.REAL, lab, nl)
    return tab, pa, pb, ra, rb, _freeze(ref)
  return _cached(('table', K, bf16), make)


def _table_args(cuda, K, dt):
  bf16 = dt == 'bf16'
  tab, pa, pb, ra, rb, ref = _table_case(K, bf16)
  g = nat.TableGraph(tab, K, cuda)
  dev = lambda p: _dev(p, cuda, bf16)
  return bf16, g, dev(pa), dev(pb), dev(ra), dev(rb), ref


TABLE = [(0, 'f32'), (0, 'bf16'), (2, 'f32'), (2, 'bf16')]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('K,dt', TABLE)
def test_table_forward_and_viterbi(cuda, K, dt, mode):
  """lt_table_forward (dist and the whole alpha), lt_table_num_forward and
  lt_table_viterbi."""
  bf16, g, da, db, ra, rb, ref = _table_args(cuda, K, dt)
  for s in (LOG, MAX, REAL):
    a, b = (ra, rb) if s == REAL else (da, db)
    d, al = _run(mode, lambda p: nat.table_forward(g, p[0], p[1], s), a, b)
    num = _run(mode, lambda p: nat.table_num_forward(g, *p, s), a, b)
    rd, ral = ref['fwd', s]
    if s == MAX:
      np.testing.assert_array_equal(_np(d), rd)
      np.testing.assert_array_equal(_np(al), ral)
      np.testing.assert_array_equal(_np(num), ref['num', s])
    elif s == LOG:
      assert_loss_close(_np(d), rd)
      assert_values_close(_np(al), ral, rtol=1e-4, atol=1e-4)
      assert_loss_close(_np(num), ref['num', s])
    else:
      _assert_real_close(_np(d), rd)
      _assert_real_close(_np(num), ref['num', s])
      _assert_real_close(_np(al), ral)  # partial distances: the distance's own bound
  for conv in (0, 1):
    labels, w = _run(mode, lambda p: nat.table_viterbi(g, p[0], p[1], conv), da, db)
    rlab, rw = ref['vit', conv]
    np.testing.assert_array_equal(_np(w), rw)
    np.testing.assert_array_equal(labels.cpu().numpy(), rlab)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('K,dt', TABLE)
def test_table_loss_grad(cuda, K, dt, mode):
  bf16, g, da, db, _, _, ref = _table_args(cuda, K, dt)
  for local in (False, True):
    loss, lz, num, dW = _run(mode, lambda p: nat.table_loss_grad(g, *p, local), da, db)
    rl, rlz, rnum, rdW = ref['loss', local]
    assert_loss_close(_np(loss), rl)
    assert_loss_close(_np(num), rnum)
    if local:  # no denominator: the header's log_z = 0, exactly
      np.testing.assert_array_equal(_np(lz), np.zeros_like(rl))
    else:
      assert_loss_close(_np(lz), rlz)
    assert_grad_marginal_close(_np(dW), rdW, None if local else ref['den'], rlz, rnum, bf16)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('K,dt', TABLE)
def test_table_den_and_num_backward(cuda, K, dt, mode):
  """lt_table_den_backward in Log, MaxTropical and Real (bf16 is the case with
  a workspace) and lt_table_num_backward in MaxTropical and Real."""
  bf16, g, da, db, ra, rb, ref = _table_args(cuda, K, dt)
  for s in (LOG, MAX, REAL):
    a, b = (ra, rb) if s == REAL else (da, db)

    def den(p):
      dist, alpha = nat.table_forward(g, p[0], p[1], s)
      return nat.table_den_backward(g, p[0], p[1], s, dist, alpha)

    dW = _np(_run(mode, den, a, b))
    if s == LOG:
      assert_grad_marginal_close(dW, ref['den'], ref['den'], ref['fwd', LOG][0], None, bf16)
    elif s == MAX:
      np.testing.assert_array_equal(dW, ref['den_grad', MAX][1])
    else:
      _assert_real_grad_close(dW, ref['den_grad', REAL][1], bf16)
    if s == LOG:
      continue
    num, dW = _run(mode, lambda p: nat.table_num_backward(g, *p, s), a, b)
    rd, rg = ref['num_grad', s]
    if s == MAX:
      np.testing.assert_array_equal(_np(num), rd)
      np.testing.assert_array_equal(_np(dW), rg)
    else:
      np.testing.assert_allclose(_np(num), rd, rtol=1e-4, atol=1e-30)
      _assert_real_grad_close(_np(dW), rg, bf16)


# ---------------------------------------------------------------------------
# lt_table_align, lt_table_sample, lt_table_expectation
# ---------------------------------------------------------------------------
ALIGN = {
    # name: C (random table) or None (bigram), V, K, B, T, U
    'table_c17_v6': (17, 6, 0, 6, 30, 9),
    'fld_k2': (None, 4, 2, 6, 20, 12),
    # 5200 x 256 decision bits exceed LDS: they go through the workspace
    'bigram_v4_t5200': (None, 4, 0, 3, 5200, 255),
}


def _align_case(name):
  def make():
    orc = _orc()
    C, V, K, B, T, U = ALIGN[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    tab = (orc.full_ngram_table(V, 1) if C is None
           else rng.integers(0, C, (C, V)).astype(np.int32))
    out = []
    for i in range(2):
      if B == 3:
        W = rng.integers(-3, 4, (B, T, tab.shape[0], V + 1)).astype(np.float32)  # ties everywhere
        nf, nl = np.array([T, 0, 1], np.int32), np.array([U, 0, 1], np.int32)
        if i == 0:
          nf, nl = nf[::-1].copy(), nl[::-1].copy()
        lab = rng.integers(1, V + 1, (B, U)).astype(np.int32)
        out.append((W, nf, lab, nl))
      else:
        out.append(_table_problem(rng, tab, B, T, U, K, False))
    W, nf, lab, nl = out[1]
    rd, rg = orc.tab_dist_grad(tab, W, nf, K, orc.MAX, lab, nl)
    assert np.isfinite(rd).any()
    ref_labels, ref_frames = align_compact.compact(rg, rd, lab, nl, nf, K)
    return tab, out[0], out[1], _freeze({'ref': (ref_labels, ref_frames, rd)})
  return _cached(('align', name), make)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', list(ALIGN))
def test_table_align(cuda, name, mode):
  """alignment_labels (0 on padding frames and unaligned rows), label_frames
  (-1 beyond num_labels) and path weights, all exact."""
  tab, pa, pb, ref = _align_case(name)
  g = nat.TableGraph(tab, ALIGN[name][2], cuda)
  labels, frames, dist = _run(mode, lambda p: nat.table_align(g, *p), _dev(pa, cuda, False),
                              _dev(pb, cuda, False))
  ref_labels, ref_frames, rd = ref['ref']
  np.testing.assert_array_equal(_np(dist), rd)
  np.testing.assert_array_equal(labels.cpu().numpy(), ref_labels)
  np.testing.assert_array_equal(frames.cpu().numpy(), ref_frames)


@pytest.mark.parametrize('mode', MODES)
def test_table_sample(cuda, mode):
  """test_gpu_sample.py's smallest replay case, ragged: labels are 0 on padding
  frames and for the empty utterance, every path walks the table with its
  weight, and every step replays from the float64 alpha and the Philox noise."""
  B, T, C, V, S = 4, 30, 17, 6, 5
  seed = 0x5eed0000cafe
  rng = np.random.default_rng(1706)
  tab = sample_ref.random_table(rng, C, V).numpy()
  g = nat.TableGraph(tab, 0, cuda)
  probs = []
  for nf in ([1, T, 0, T - 1], [T, T - 1, 1, 0]):
    W = rng.standard_normal([B, T, C, V + 1]).astype(np.float32)
    probs.append((W, np.array(nf, np.int32)))

  def fn(p):
    log_z, alpha = nat.table_forward(g, p[0], p[1], LOG)
    labels, weights = nat.table_sample(g, p[0], p[1], log_z, alpha, S, seed)
    return labels, weights, log_z

  da, db = ((torch.tensor(W).to(cuda), torch.tensor(nf).to(cuda)) for W, nf in probs)
  labels, weights, log_z = (x.cpu().numpy() for x in _run(mode, fn, da, db))
  W, nf = probs[1]
  want_z, alpha = sample_ref.forward(W, nf, tab)
  np.testing.assert_allclose(log_z, want_z, rtol=1e-4, atol=1e-4)
  sample_ref.check_paths(W, nf, tab, labels, weights, log_z)
  steps, _ = sample_ref.replay(W, nf, tab, labels, seed, alpha)
  assert steps == S * int(nf.sum())
  assert not labels[3].any() and not weights[3].any()  # num_frames = 0: the empty path
  # the seeded paths are cpu.sample's (the header's definition in torch ops) on the same alpha
  import last_torch_amd as lt
  from last_torch_amd import cpu as cpu_path
  lz, al = nat.table_forward(g, db[0], db[1], LOG)
  want, _, _ = cpu_path.sample(db[0], db[1], lt.contexts.NextStateTable(torch.tensor(tab)), S, seed,
                            log_z=lz, alpha=al)
  np.testing.assert_array_equal(labels, want.cpu().numpy())


@pytest.mark.parametrize('mode', MODES)
def test_table_expectation(cuda, mode):
  """E, log_z and both gradient tensors (0 on padding frames) against
  cpu.expectation in float64, under test_gpu_expectation.py's bounds."""
  import last_torch_amd as lt

  def make():
    rng = np.random.default_rng(5)
    context = lt.contexts.NextStateTable(expect_ref.random_table(rng, 17, 6))
    T, B = 30, 4
    g = torch.Generator().manual_seed(4)
    out = []
    for nf in ([1, T, 0, T - 1], [T, T - 1, 1, 0]):
      W = torch.randn([B, T, 17, 7], generator=g) - 2
      v = torch.randn([B, T, 17, 7], generator=g)
      out.append((W, v, nf))
    W, v, nf = out[1]
    r64 = expect_ref.cpu_reference(W, v, nf, context, b=torch.zeros(B))
    r32 = expect_ref.cpu_reference(W, v, nf, context, b=torch.zeros(B), dtype=torch.float32)
    return context, out[0], out[1], r64, float(np.abs(r32['dW'] - r64['dW']).max())

  context, pa, pb, r64, e32 = _cached(('expect',), make)
  graph = nat.TableGraph(context.next_state_table.numpy(), 0, cuda)
  dev = lambda p: (p[0].to(cuda), p[1].to(cuda), torch.tensor(p[2], dtype=torch.int32, device=cuda))
  out = _run(mode, lambda p: nat.table_expectation(graph, *p), dev(pa), dev(pb))
  E, log_z, marg, cov = (x.double().cpu().numpy() for x in out)
  np.testing.assert_allclose(log_z, r64['log_z'], rtol=1e-4, atol=1e-4)
  np.testing.assert_allclose(E, r64['E'], rtol=1e-4, atol=1e-4)
  marg_atol = 1e-5 * max(1.0, float(np.abs(r64['dv']).max()))
  assert (np.abs(marg - r64['dv']) <= marg_atol + 1e-4 * np.abs(r64['dv'])).all()
  cov_bound = np.maximum(4 * e32, marg_atol + 1e-4 * np.abs(r64['dW']))
  assert (np.abs(cov - r64['dW']) <= cov_bound).all()
  nf = pb[2]
  for b in range(4):  # padding frames and the empty utterance: exact zeros
    assert not marg[b, nf[b]:].any() and not cov[b, nf[b]:].any()
  assert E[3] == 0 and log_z[3] == 0


# ---------------------------------------------------------------------------
# the joint weight function (lt_producer.hip) and its fusion into the loss
# (lt_joint.hip)
# ---------------------------------------------------------------------------
def _joint_ref(pc, pf, wo, bias):
  """The fp32 PyTorch restatement of test_gpu_producer.py."""
  hid = torch.tanh(pc[None] + pf.reshape(-1, pf.shape[-1])[:, None, :])
  return (torch.matmul(hid, wo.t()) + bias).reshape(*pf.shape[:-1], pc.shape[0], wo.shape[0])


def _joint_tol(pc, pf, wo):
  hid = torch.tanh(pc[None] + pf.reshape(-1, pf.shape[-1])[:, None, :]).abs()
  return 2.0 ** -7 * torch.matmul(hid, wo.abs().t()).reshape(
      *pf.shape[:-1], pc.shape[0], wo.shape[0]) + 1e-5


def _joint_inputs(cuda, lead, C, H, R, seed):
  g = torch.Generator(device=cuda)
  g.manual_seed(seed)
  pc = torch.randn([C, H], generator=g, device=cuda)
  pf = torch.randn([*lead, H], generator=g, device=cuda)
  wo = torch.randn([R, H], generator=g, device=cuda) / H ** 0.5
  bias = torch.randn([R], generator=g, device=cuda)
  return pc, pf, wo, bias


JOINT = dict(lead=(2, 24), C=33, H=64, R=33)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_joint_weights(cuda, precision, mode):
  a, b = (_joint_inputs(cuda, seed=s, **JOINT) for s in (1, 2))
  W = _run(mode, lambda p: nat.joint_weights(*p, precision=precision), a, b)
  ref = _joint_ref(*b)
  tol = _joint_tol(*b[:3])
  if precision == 'fp32':
    tol = tol * 2.0 ** -7 + 1e-5
  assert W.shape == ref.shape
  assert bool(((W - ref).abs() <= tol).all())  # a NaN fails the comparison


@pytest.mark.parametrize('mode', MODES)
def test_joint_weights_backward(cuda, mode):
  C, H, R = JOINT['C'], JOINT['H'], JOINT['R']
  assert nat.joint_weights_backward_supported(C, H, R)
  probs = []
  for s in (3, 4):
    pc, pf, wo, bias = _joint_inputs(cuda, seed=s, **JOINT)
    g = torch.randn([*JOINT['lead'], C, R], device=cuda,
                    generator=torch.Generator(device=cuda).manual_seed(s))
    probs.append((pc, pf, wo, g, bias))
  got = _run(mode, lambda p: nat.joint_weights_backward(*p[:4]), *probs)
  pc, pf, wo, g, bias = probs[1]
  leaves = [t.clone().requires_grad_(True) for t in (pc, pf, wo, bias)]
  (_joint_ref(*leaves) * g).sum().backward()
  for name, x, leaf in zip(('pc', 'pf', 'wo', 'bias'), got, leaves):
    scale = float(leaf.grad.abs().max())
    err = float((x - leaf.grad).abs().max())
    assert err <= 1e-4 * max(1.0, scale), (name, err, scale)  # a NaN fails the comparison


def _joint_loss_case(cuda):
  def make():
    orc = _orc()
    B, T, U, H, V = 6, 24, 6, 64, 32
    out = []
    for seed in (8, 9):
      g = torch.Generator(device=cuda)
      g.manual_seed(seed)
      pc = torch.randn([V + 1, H], generator=g, device=cuda) * 0.5
      pf = torch.randn([B, T, H], generator=g, device=cuda) * 0.5
      wo = torch.randn([V + 1, H], generator=g, device=cuda) * (2.0 / math.sqrt(H))
      bias = torch.randn([V + 1], generator=g, device=cuda) * 0.1
      rng = np.random.default_rng(seed)
      nf, nl = _lengths(B, T, U)
      perm = rng.permutation(B)
      lab = rng.integers(0, V + 1, (B, U)).astype(np.int32)  # epsilons included
      out.append((pc, pf, wo, bias, torch.tensor(nf[perm].copy(), device=cuda),
                  torch.tensor(lab, device=cuda), torch.tensor(nl[perm].copy(), device=cuda)))
    pc, pf, wo, bias, nf, lab, nl = out[1]
    # the oracle on the materialised W, its dW pulled back through fp32
    # autograd of the reference formulation (test_gpu_joint_fused.py)
    W = nat.joint_weights(pc, pf, wo, bias, precision='fp32')
    rl, rlz, rnum, rdW = orc.loss_grad(W.cpu().numpy(), nf.cpu().numpy(), lab.cpu().numpy(),
                                       nl.cpu().numpy(), V, 1)
    assert np.isposinf(rl).any()
    ps = [x.clone().requires_grad_(True) for x in (pc, pf, wo, bias)]
    hid = torch.tanh(ps[0][None, None] + ps[1][:, :, None, :])
    ((hid @ ps[2].t() + ps[3]) * torch.from_numpy(rdW).to(cuda)).sum().backward()
    return out[0], out[1], (rl, rlz, rnum), [p.grad for p in ps]
  return _cached(('joint_loss',), make)


def _check_joint(loss, lz, num, grads, ref, ref_grads):
  rl, rlz, rnum = ref
  assert_loss_close(_np(loss), rl)
  assert_loss_close(_np(lz), rlz)
  assert_loss_close(_np(num), rnum)
  for got, want in zip(grads, ref_grads):
    scale = float(want.abs().max()) + 1e-30
    err = float((got - want).abs().max())
    assert err <= 1e-3 * scale, (err, scale)  # a NaN fails the comparison


@pytest.mark.parametrize('mode', MODES)
def test_loss_grad_joint(cuda, mode):
  pa, pb, ref, ref_grads = _joint_loss_case(cuda)
  assert nat.joint_loss_supported(6, 24, 6, 32, 1, 64)
  out = _run(mode, lambda p: nat.loss_grad_joint(*p), pa, pb)
  _check_joint(out[0], out[1], out[2], out[3:], ref, ref_grads)


@pytest.mark.parametrize('mode', MODES)
def test_joint_loss_forward_backward(cuda, mode):
  pa, pb, ref, ref_grads = _joint_loss_case(cuda)

  def fn(p):
    loss, lz, num, state = nat.joint_loss_forward(*p)
    return loss, lz, num, nat.joint_loss_backward(*p[:6], state)

  loss, lz, num, grads = _run(mode, fn, pa, pb)
  _check_joint(loss, lz, num, grads, ref, ref_grads)


# ---------------------------------------------------------------------------
# the fused pipe's stale tags
# ---------------------------------------------------------------------------
def test_fused_pipe_stale_tags(cuda):
  """In a fresh process (the pipe's epoch counter starts at zero) problem A
  with 2T frames, then problem B with T frames in the same workspace:
  utterance 0's granules hold A's tags 2T + t', which are the tags B's epoch
  expects (pipe_stale_child.py)."""
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'pipe_stale_child.py')],
                     cwd=ROOT, capture_output=True, text=True, timeout=280)
  assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
  assert r.stdout.startswith('ok'), r.stdout[-2000:]
