"""The general table kernels (lt_table.hip) on every shape-selected path the
host code at the bottom of that file can take, against the pinned table
oracle (oracle/table_oracle.c):

* 256 against 512 threads and one, two or three passes of the 8-lanes-per-
  state reductions (C around 32, 64, 128);
* the staged, half-staged and unstaged variants (STAGE, `acc`), with a pure-
  Python mirror of the host's predicates that a test WITHOUT the gpu mark
  holds against the shapes used here, so a moved budget names the shape to
  move on a CPU-only host;
* the dense-bigram FrameLabelDependent kernels (tab_fwd_dense[2],
  tab_bwd_den_dense[2]) around the half-wave split at 17 sources, at V = 32,
  at K <= and > kTabDenseKMax, in bf16, and on tables that only look like
  the bigram's;
* in-degrees of 0, 1..7, 8, 9.. and C * V;
* the Viterbi backtrace over more than one LDS chunk, with and without the
  in-arc table in LDS, and (diagnostic build, tests/diag_table_child.py) the
  serial backtrace and 512 threads on few states;
* the string side at long transcripts, the MaxTropical string walk over two
  decision chunks, and the host's refusal where the string rows stop fitting
  in LDS.

Tolerances are the project's (golden_cases.py, test_gpu_table.py,
test_gpu_string_grad.py); nothing is introduced here.
"""
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

from last_torch_amd import _native as nat
from golden_cases import (assert_grad_marginal_close, assert_loss_close, assert_values_close,
                          table_den_marginals)
from test_gpu_string_grad import assert_real_grad_close
from test_gpu_table import SID, _orc

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG = os.path.join(ROOT, 'build', 'diag', 'liblt_lattice_diag.so')

# ---------------------------------------------------------------------------
# Mirror of the host's dispatch predicates (last_torch_amd/csrc/lt_table.hip,
# "host side"; the constants from lt_table_common.h). Each function names the
# lines it copies; lt_table.hip names this module at each of them.
# ---------------------------------------------------------------------------
K_TAB_LDS = 160 * 1024       # lt_table_common.h kTabLds
K_STAGE_BUDGET = 144 * 1024  # lt_table_common.h kStageBudget
K_STR_CHUNK = 32768          # lt_table.hip kStrChunk
K_BT_BUDGET = 60 * 1024      # lt_table_viterbi: `budget`


def fwd_lds(S):  # lt_table.hip fwd_lds()
  return 4 * (4 * S) + 8 * S


def graph_lds(C, V):  # lt_table.hip graph_lds()
  return 4 * ((C + 1 + 2 * C * V + 3) // 4 * 4)


def tab_threads(C):  # lt_table.hip tab_threads()
  return 512 if C > 32 else 256


def fwd_staged(C, V, K):  # launch_t_fwd / lt_table_loss_grad: `staged <= kStageBudget`
  FR = C * (V + 1)
  return fwd_lds(C) + graph_lds(C, V) + (8 if K == 0 else 4) * FR <= K_STAGE_BUDGET


def _lds_d(C, K):  # lt_table_loss_grad / lt_table_den_backward: lds_d
  return 4 * (3 * C + (K + 1) * C)


def bwd_staged(C, V, K):  # lt_table_loss_grad / lt_table_den_backward: the staged branch
  FR = C * (V + 1)
  return _lds_d(C, K) + graph_lds(C, V) + (8 if K == 0 else 4) * FR <= K_STAGE_BUDGET


def bwd_acc(C, V, K):  # lt_table_loss_grad / lt_table_den_backward: ad.acc / a.acc
  FR = C * (V + 1)
  return bwd_staged(C, V, K) and K > 0 and _lds_d(C, K) + graph_lds(C, V) + 8 * FR <= K_STAGE_BUDGET


def backtrace_chunk(C, V, K, T):
  """lt_table_viterbi: (frames per LDS chunk, arcs_lds); chunk 0 = the serial
  tab_backtrace_kernel."""
  KK = K if K > 0 else 1
  per_frame = 4 * KK * C + (C if K > 0 else 0)
  arcs_bytes = 4 * C * V
  arcs_lds = arcs_bytes <= K_BT_BUDGET // 2
  room = K_BT_BUDGET - (arcs_bytes if arcs_lds else 0)
  return min(max(1, T), room // per_frame), arcs_lds


def str_grad_lds(U, K, maxt):  # lt_table.hip str_grad_lds()
  S = U + 1
  return (4 * (5 * S + (9 + K + 1 + 2) * S + 4 + ((K + 1 + 3) & ~3) * 2) +
          (max(K_STR_CHUNK, S) if maxt else 0))


def str_walk_frames(U):  # tab_str_grad_kernel: F, frames per decision chunk
  return max(1, K_STR_CHUNK // (U + 1))


def loss_grad_lds_n(U, K):  # lt_table_loss_grad: lds_n (the string backward's rows)
  S = U + 1
  return 4 * (8 * S + (K + 1) * S) + 4 * (2 * S + 2 * S) + 4 * (2 * S + 2 * S) + (12 * S if K == 0 else 0)


def num_fwd_lds(U):  # launch_t_fwd with num: fwd_lds(S) + 16 S
  return fwd_lds(U + 1) + 16 * (U + 1)


def regime(C, V, K):
  return (fwd_staged(C, V, K), bwd_staged(C, V, K), bwd_acc(C, V, K))


# V = 28, T = 10, B = 2: (K, C, dtype) -> (forward staged, backward staged, acc)
STAGING = [
    (0, 300, 'f32', (True, True, False)),    # staged forward and backward
    (0, 305, 'f32', (False, True, False)),   # unstaged forward, staged backward
    (0, 320, 'f32', (False, False, False)),  # unstaged forward and backward
    (2, 300, 'f32', (True, True, True)),     # staged with acc
    (2, 320, 'f32', (True, True, False)),    # staged without acc
    (2, 410, 'f32', (False, False, False)),  # unstaged
    (0, 300, 'bf16', (True, True, False)),
    (2, 410, 'bf16', (False, False, False)),
]
STAGING_V = 28

# C, V, K, T -> more than one backtrace chunk; arcs in LDS or not
BACKTRACE = [
    (65, 3, 0, 240, True),
    (320, 28, 0, 50, False),
    (410, 28, 2, 20, False),
]


def test_dispatch_mirror_places_every_shape():
  """Without a GPU: every shape this module uses to reach a regime falls in
  that regime under the mirrored predicates. A failure names the shape whose
  C has to move after a budget changed in lt_table.hip."""
  for K, C, _, want in STAGING:
    assert regime(C, STAGING_V, K) == want, (
        f'K={K} C={C} V={STAGING_V}: (fwd staged, bwd staged, acc) = '
        f'{regime(C, STAGING_V, K)}, this module expects {want}')
  assert {w for _, _, _, w in STAGING} == {(True, True, False), (False, True, False),
                                          (False, False, False), (True, True, True)}
  assert {(K > 0, w) for K, _, _, w in STAGING} >= {
      (False, (True, True, False)), (False, (False, True, False)), (False, (False, False, False)),
      (True, (True, True, True)), (True, (True, True, False)), (True, (False, False, False))}
  for C, V, K, T, arcs in BACKTRACE:
    chunk, arcs_lds = backtrace_chunk(C, V, K, T)
    assert arcs_lds == arcs, (C, V, K, arcs_lds)
    assert 1 <= chunk and chunk + 1 < T, f'C={C} V={V} K={K} T={T}: one chunk of {chunk} frames'
  assert backtrace_chunk(*SERIAL_BACKTRACE, 3)[0] == 0
  assert backtrace_chunk(59, 1, 255, 3)[0] == 1  # (a few states fewer still fit a frame)
  # every other case of this module is far inside the staged regime
  for C, V, K in [(129, 3, 2), (34, 33, 4), (33, 32, 5), (70, 2, 1), (65, 9, 1)]:
    assert regime(C, V, K)[:2] == (True, True), (C, V, K)
  assert [tab_threads(C) for C in (32, 33)] == [256, 512]
  # the MaxTropical string walk of test_string_walk_two_chunks
  assert str_walk_frames(255) == 128
  # the refusals of test_string_side_refused_past_lds sit exactly on the rule
  for maxt in (True, False):
    U = _first_refused(lambda u: str_grad_lds(u, 0, maxt))
    assert str_grad_lds(U - 1, 0, maxt) <= K_TAB_LDS < str_grad_lds(U, 0, maxt)
  assert _first_refused(lambda u: str_grad_lds(u, 0, True)) == 1926
  assert _first_refused(lambda u: loss_grad_lds_n(u, 0)) == 2048
  assert _first_refused(num_fwd_lds) == 4096


def _first_refused(lds_of_u):
  """Smallest U whose LDS need passes kTabLds (the needs grow with U)."""
  lo, hi = 0, 1 << 20
  while lo < hi:
    mid = (lo + hi) // 2
    if lds_of_u(mid) > K_TAB_LDS:
      hi = mid
    else:
      lo = mid + 1
  return lo


# ---------------------------------------------------------------------------
# The checker
# ---------------------------------------------------------------------------
ALL = frozenset({'forward', 'num_forward', 'loss_grad', 'den_backward', 'num_backward', 'viterbi',
                 'real'})


def draw_problem(table, K, B, T, U, dtype, rng, nf=None, nl=None):
  """N(0,1) W (through bf16 for bf16), num_frames with T, 1 and 0 and
  num_labels with U, one unreachable value (U labels on the one-frame
  utterance, when U > max(1, K)) and 0 -- with B = 2 the second utterance
  draws one of the two short ones --, labels with epsilons, and -inf on about
  2 % of utterance 0's lexical arcs."""
  table = np.ascontiguousarray(table, np.int32)
  C, V = table.shape
  bf16 = dtype == 'bf16'
  W = rng.standard_normal((B, T, C, V + 1)).astype(np.float32)
  if bf16:
    W = torch.tensor(W).bfloat16().float().numpy()
  W[0, :, :, 1:][rng.random((T, C, V)) < 0.02] = -np.inf
  short = [(1, U), (0, 0)]
  if B == 2:
    short = [short[int(rng.integers(0, 2))]]
  own_nf = nf is None
  if own_nf:
    nf = rng.integers(0, T + 1, B)
    nf[0] = T
  if nl is None:
    nl = rng.integers(0, U + 1, B)
    nl[0] = U
    if own_nf:
      for i, (f, l) in enumerate(short[:B - 1]):
        nf[1 + i], nl[1 + i] = f, l
  lab = rng.integers(0, V + 1, (B, U)).astype(np.int32)
  if U > 1:
    lab[0, U // 2] = 0
  return dict(table=table, K=K, C=C, V=V, B=B, T=T, U=U, bf16=bf16, W=W,
              nf=np.asarray(nf, np.int32), lab=lab, nl=np.asarray(nl, np.int32),
              gin=np.linspace(0.5, 2.0, B).astype(np.float32))


def real_problem(p):
  """The Real semiring's weights (test_gpu_string_grad.py): 12 frames of
  exp(W - log(V + 1)) * 1.3, so that alpha stays inside fp32."""
  Tr = min(p['T'], 12)
  Wr = (np.exp(p['W'][:, :Tr] - np.log(p['V'] + 1.0)) * 1.3).astype(np.float32)
  if p['bf16']:
    Wr = torch.tensor(Wr).bfloat16().float().numpy()
  return np.ascontiguousarray(Wr), np.minimum(p['nf'], Tr).astype(np.int32)


def reference(p, parts=ALL):
  """Everything the checker compares, from the oracle (no GPU)."""
  orc = _orc()
  tab, K, W, nf, lab, nl, gin = (p[k] for k in ('table', 'K', 'W', 'nf', 'lab', 'nl', 'gin'))
  r = {}
  if 'forward' in parts or 'den_backward' in parts:
    for s, sid in (('Log', orc.LOG), ('MaxTropical', orc.MAX)):
      r['den', s] = orc.tab_den_forward(tab, W, nf, K, sid, want_alpha=True)
  if 'num_forward' in parts:
    for s, sid in (('Log', orc.LOG), ('MaxTropical', orc.MAX)):
      r['num', s] = orc.tab_num_forward(tab, W, nf, lab, nl, K, sid)
  if 'loss_grad' in parts or 'den_backward' in parts:
    r['den_marg'] = table_den_marginals(orc, tab, W, nf, lab, nl, K)
  if 'loss_grad' in parts:
    for local in (False, True):
      r['loss_grad', local] = orc.tab_loss_grad(tab, W, nf, lab, nl, K, local_norm=local)
  if 'den_backward' in parts:
    r['den_grad', 'MaxTropical'] = orc.tab_dist_grad(tab, W, nf, K, orc.MAX, grad=gin)
  if 'num_backward' in parts:
    r['num_grad', 'MaxTropical'] = orc.tab_dist_grad(tab, W, nf, K, orc.MAX, lab, nl, grad=gin)
  if 'viterbi' in parts:
    for conv in (0, 1):
      r['viterbi', conv] = orc.tab_viterbi(tab, W, nf, K, conv)
  if 'real' in parts:
    Wr, nfr = real_problem(p)
    r['den', 'Real'] = orc.tab_den_forward(tab, Wr, nfr, K, orc.REAL)
    r['num', 'Real'] = orc.tab_num_forward(tab, Wr, nfr, lab, nl, K, orc.REAL)
    r['den_grad', 'Real'] = orc.tab_dist_grad(tab, Wr, nfr, K, orc.REAL, grad=gin)
    r['num_grad', 'Real'] = orc.tab_dist_grad(tab, Wr, nfr, K, orc.REAL, lab, nl, grad=gin)
    for k in (('den', 'Real'), ('num', 'Real')):
      assert np.isfinite(r[k]).all()
    for k in (('den_grad', 'Real'), ('num_grad', 'Real')):
      assert np.isfinite(r[k][0]).all() and np.isfinite(r[k][1]).all()
  return r


def _np(x):
  return x.float().cpu().numpy()


def _assert_real_grad(got, ref, bf16):
  if bf16:  # dW rounded to bf16: 2^-8 relative (test_gpu_string_grad.py)
    np.testing.assert_allclose(got, ref, rtol=2 ** -8 + 1e-4, atol=1e-30)
  else:
    assert_real_grad_close(got, ref)


def check_table_paths(cuda, table, K, B, T, U, dtype, rng, parts=ALL, nf=None, nl=None):
  """Draws a problem (draw_problem) and holds the table entry points named in
  `parts` against the oracle. Returns the problem."""
  p = draw_problem(table, K, B, T, U, dtype, rng, nf=nf, nl=nl)
  r = reference(p, parts)
  bf16 = p['bf16']
  tdt = torch.bfloat16 if bf16 else torch.float32
  g = nat.TableGraph(p['table'], K, cuda)
  Wd = torch.tensor(p['W']).to(tdt).to(cuda)
  nfd, labd, nld = (torch.tensor(p[k]).to(cuda) for k in ('nf', 'lab', 'nl'))
  gind = torch.tensor(p['gin']).to(cuda)
  fwd = {}
  if 'forward' in parts or 'den_backward' in parts:
    for s in ('Log', 'MaxTropical'):
      d, a = nat.table_forward(g, Wd, nfd, SID[s])
      fwd[s] = (d, a)
      rd, ra = r['den', s]
      if s == 'MaxTropical':
        np.testing.assert_array_equal(_np(d), rd)
        np.testing.assert_array_equal(_np(a), ra)
      else:
        assert_loss_close(_np(d), rd)
        assert_values_close(_np(a), ra, rtol=1e-4, atol=1e-4)
      d2, _ = nat.table_forward(g, Wd, nfd, SID[s], want_alpha=False)
      np.testing.assert_array_equal(_np(d2), _np(d))
  if 'num_forward' in parts:
    for s in ('Log', 'MaxTropical'):
      num = _np(nat.table_num_forward(g, Wd, nfd, labd, nld, SID[s]))
      if s == 'MaxTropical':
        np.testing.assert_array_equal(num, r['num', s])
      else:
        assert_loss_close(num, r['num', s])
  if 'loss_grad' in parts:
    for local in (False, True):
      loss, lz, num, dW = nat.table_loss_grad(g, Wd, nfd, labd, nld, local)
      rl, rlz, rnum, rdW = r['loss_grad', local]
      assert_loss_close(_np(loss), rl)
      assert_loss_close(_np(num), rnum)
      if not local:
        assert_loss_close(_np(lz), rlz)
      assert_grad_marginal_close(_np(dW), rdW, None if local else r['den_marg'], rlz, rnum, bf16)
  if 'den_backward' in parts:
    d, a = fwd['Log']
    dW = nat.table_den_backward(g, Wd, nfd, SID['Log'], dist=d, alpha=a)
    den = r['den_marg']
    assert_grad_marginal_close(_np(dW), den, den, r['den', 'Log'][0], None, bf16)
    dW = nat.table_den_backward(g, Wd, nfd, SID['MaxTropical'], grad=gind)
    np.testing.assert_array_equal(_np(dW), r['den_grad', 'MaxTropical'][1])
  if 'num_backward' in parts:
    num, dW = nat.table_num_backward(g, Wd, nfd, labd, nld, SID['MaxTropical'], grad=gind)
    rd, rg = r['num_grad', 'MaxTropical']
    np.testing.assert_array_equal(_np(num), rd)
    np.testing.assert_array_equal(_np(dW), rg)
  if 'viterbi' in parts:
    for conv in (0, 1):
      labels, w = nat.table_viterbi(g, Wd, nfd, conv)
      rlab, rw = r['viterbi', conv]
      np.testing.assert_array_equal(_np(w), rw)
      np.testing.assert_array_equal(labels.cpu().numpy(), rlab)
  if 'real' in parts:
    Wr, nfr = real_problem(p)
    Wrd = torch.tensor(Wr).to(tdt).to(cuda)
    nfrd = torch.tensor(nfr).to(cuda)
    d, a = nat.table_forward(g, Wrd, nfrd, SID['Real'])
    np.testing.assert_allclose(_np(d), r['den', 'Real'], rtol=1e-4, atol=1e-30)
    num = nat.table_num_forward(g, Wrd, nfrd, labd, nld, SID['Real'])
    np.testing.assert_allclose(_np(num), r['num', 'Real'], rtol=1e-4, atol=1e-30)
    dW = nat.table_den_backward(g, Wrd, nfrd, SID['Real'], dist=d, alpha=a, grad=gind)
    _assert_real_grad(_np(dW), r['den_grad', 'Real'][1], bf16)
    num, dW = nat.table_num_backward(g, Wrd, nfrd, labd, nld, SID['Real'], grad=gind)
    np.testing.assert_allclose(_np(num), r['num_grad', 'Real'][0], rtol=1e-4, atol=1e-30)
    _assert_real_grad(_np(dW), r['num_grad', 'Real'][1], bf16)
  return p


def _rng(*key):
  return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _random_table(rng, C, V):
  return rng.integers(0, C, (C, V)).astype(np.int32)


# ---------------------------------------------------------------------------
# 1. state-count boundaries: 256 | 512 threads, one | two | three passes
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('K', [0, 2])
@pytest.mark.parametrize('C', [32, 33, 64, 65, 129])
def test_state_count_boundaries(cuda, C, K):
  rng = _rng('states', C, K)
  check_table_paths(cuda, _random_table(rng, C, 3), K, 3, 12, 5, 'f32', rng)


# ---------------------------------------------------------------------------
# 2. staging regimes (test_dispatch_mirror_places_every_shape holds the table)
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('K,C,dt', [c[:3] for c in STAGING],
                         ids=[f'k{c[0]}_c{c[1]}_{c[2]}' for c in STAGING])
def test_staging_regimes(cuda, K, C, dt):
  rng = _rng('staging', K, C, dt)
  check_table_paths(cuda, _random_table(rng, C, STAGING_V), K, 2, 10, 6, dt, rng)


# ---------------------------------------------------------------------------
# 3. the dense-bigram FrameLabelDependent kernels
# ---------------------------------------------------------------------------
DENSE = ([(V, K, 'f32') for V in (1, 2, 15, 16, 17, 18, 31, 32) for K in (1, 4)] +
         [(V, 5, 'f32') for V in (17, 32)] +   # dense forward, generic backward
         [(V, 2, 'bf16') for V in (17, 32)])


@gpu
@pytest.mark.parametrize('V,K,dt', DENSE, ids=[f'v{v}_k{k}_{d}' for v, k, d in DENSE])
def test_dense_bigram(cuda, V, K, dt):
  rng = _rng('dense', V, K, dt)
  check_table_paths(cuda, _orc().full_ngram_table(V, 1), K, 3, 9, 6, dt, rng)


@gpu
@pytest.mark.parametrize('K', [1, 4])
@pytest.mark.parametrize('which', ['v33_too_wide', 'v32_last_entry_changed'])
def test_bigram_lookalikes_take_the_generic_path(cuda, which, K):
  """C = V + 1 tables the dense kernels must leave alone: V = 33, and the
  V = 32 bigram with its last entry (the one a short bound in
  tab_dense_bigram's strided check would miss) sent to another state."""
  orc = _orc()
  if which == 'v33_too_wide':
    table = orc.full_ngram_table(33, 1)
  else:
    table = orc.full_ngram_table(32, 1).copy()
    assert table[-1, -1] == 32
    table[-1, -1] = 5
  rng = _rng('lookalike', which, K)
  check_table_paths(cuda, table, K, 3, 9, 6, 'f32', rng)


# ---------------------------------------------------------------------------
# 4. skewed in-degrees
# ---------------------------------------------------------------------------
def _in_degree_ramp():
  """C = 17, V = 8: state q has exactly q in-arcs (sum 136 = C * V)."""
  C, V = 17, 8
  dest = np.repeat(np.arange(C), np.arange(C))
  assert dest.size == C * V
  # spread each state's in-arcs over sources and labels
  table = np.empty(C * V, np.int32)
  table[np.random.default_rng(17).permutation(C * V)] = dest
  table = table.reshape(C, V)
  assert (np.bincount(table.ravel(), minlength=C) == np.arange(C)).all()
  return table


def _skew_table(name):
  if name == 'ramp_0_to_16':
    return _in_degree_ramp()
  if name == 'all_into_state0':
    return np.zeros((65, 9), np.int32)
  if name == 'permutation':
    return np.random.default_rng(40).permutation(40).astype(np.int32).reshape(40, 1)
  if name == 'chain':
    C = 70
    return np.repeat(np.minimum(np.arange(C) + 1, C - 1)[:, None], 2, 1).astype(np.int32)
  raise KeyError(name)


@gpu
@pytest.mark.parametrize('K', [0, 1])
@pytest.mark.parametrize('name', ['ramp_0_to_16', 'all_into_state0', 'permutation', 'chain'])
def test_skewed_in_degrees(cuda, name, K):
  table = _skew_table(name)
  check_table_paths(cuda, table, K, 3, 10, 5, 'f32', _rng('skew', name, K))


# ---------------------------------------------------------------------------
# 5. Viterbi backtrace over more than one chunk
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('C,V,K,T', [c[:4] for c in BACKTRACE],
                         ids=[f'c{c[0]}_v{c[1]}_k{c[2]}_t{c[3]}' for c in BACKTRACE])
def test_backtrace_chunks(cuda, C, V, K, T):
  """Utterances of T frames (more than one chunk), of exactly one chunk and
  of one chunk and a frame: table_viterbi under both conventions and the
  MaxTropical den backward (which shares the Viterbi forward)."""
  chunk, _ = backtrace_chunk(C, V, K, T)
  rng = _rng('backtrace', C, V, K, T)
  check_table_paths(cuda, _random_table(rng, C, V), K, 3, T, 4, 'f32', rng,
                    parts={'viterbi', 'den_backward'}, nf=[T, chunk, chunk + 1])


# C, V, K: a frame's backpointers (4 K C + C bytes) pass the backtrace's LDS
# budget, so the product library takes the serial tab_backtrace_kernel
SERIAL_BACKTRACE = (61, 1, 255)


@gpu
def test_backtrace_serial_at_255_expansions(cuda):
  """The one shape family that reaches the serial backtrace without the
  diagnostic switch: FrameLabelDependent(K) with 4 K C + C past 60 KiB, here
  K = 255 on 61 states."""
  C, V, K = SERIAL_BACKTRACE
  assert backtrace_chunk(C, V, K, 3)[0] == 0
  rng = _rng('serial', C, V, K)
  check_table_paths(cuda, _random_table(rng, C, V), K, 3, 3, 2, 'f32', rng, parts={'viterbi'})


def _diag_child(env, timeout=120):
  assert os.path.exists(DIAG), 'diagnostic build absent (build() makes it: make diag)'
  env = dict(os.environ, LT_LIB_PATH=DIAG, **env)
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'diag_table_child.py')],
                     cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
  assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
  assert r.stdout.startswith('ok'), r.stdout[-2000:]


@gpu
@pytest.mark.parametrize('env', [{'LT_TAB_BT_SERIAL': '1'}, {'LT_TAB_THREADS': '512'}],
                         ids=['serial_backtrace', 'threads_512'])
def test_diag_switches(cuda, env):
  """The serial backtrace (tab_backtrace_kernel) and 512 threads on C = 7 and
  C = 40, which only the diagnostic build's switches select: one fresh child
  each (tests/diag_table_child.py)."""
  _diag_child(env)


# ---------------------------------------------------------------------------
# 6. long strings
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('U', [0, 1, 255, 256, 257, 600])
def test_long_strings(cuda, U):
  """T = U + 20 frames with all U labels, and a half-length utterance."""
  rng = _rng('strings', U)
  check_table_paths(cuda, _random_table(rng, 5, 3), 0, 2, U + 20, U, 'f32', rng,
                    parts={'num_forward', 'loss_grad'}, nf=[U + 20, U // 2 + 7], nl=[U, U // 2])


@gpu
def test_string_walk_two_chunks(cuda):
  """MaxTropical table_num_backward at U = 255: S = 256, 128 frames of
  decisions per chunk; utterances of 128 (one chunk), 129 and 130 frames."""
  U, T = 255, 130
  F = str_walk_frames(U)
  assert F == 128
  rng = _rng('walk')
  check_table_paths(cuda, _random_table(rng, 5, 3), 0, 3, T, U, 'f32', rng, parts={'num_backward'},
                    nf=[F, F + 1, T], nl=[F, 60, 100])


@gpu
def test_string_side_refused_past_lds(cuda):
  """Where the string rows stop fitting in LDS the host refuses
  (LT_EUNSUPPORTED -> LatticeLibraryError) in the workspace query and in the
  call, and launches nothing; a following call is served. At U0, the first U
  the mirrored rule refuses: refused. At U0 - 1 the rows fit the rule, but a
  kernel's static LDS (a few slot words, under one position's 40 to 80
  bytes) counts against the same 160 KiB: served, or refused as
  LT_EUNSUPPORTED, never a HIP error. At U0 - 2: served, and right."""
  orc = _orc()
  rng = _rng('refusal')
  table = _random_table(rng, 5, 3)
  g = nat.TableGraph(table, 0, cuda)
  B, T = 1, 2
  W = rng.standard_normal((B, T, 5, 4)).astype(np.float32)
  nf, nl = np.array([T], np.int32), np.array([1], np.int32)
  Wd, nfd, nld = (torch.tensor(x).to(cuda) for x in (W, nf, nl))
  unsupported = r'\(-2\).*exceeds? LDS'

  def num_backward(s, sid):
    def run(lab, labd):
      nat.table_num_backward_check(g, Wd, labd, SID[s])
      num, dW = nat.table_num_backward(g, Wd, nfd, labd, nld, SID[s])
      rd, rg = orc.tab_dist_grad(table, W, nf, 0, sid, lab, nl)
      if s == 'MaxTropical':
        np.testing.assert_array_equal(_np(num), rd)
        np.testing.assert_array_equal(_np(dW), rg)
      else:
        np.testing.assert_allclose(_np(num), rd, rtol=1e-4, atol=1e-30)
        assert_real_grad_close(_np(dW), rg)
    return run

  def loss_grad(lab, labd):
    loss, _, _, dW = nat.table_loss_grad(g, Wd, nfd, labd, nld, False)
    rl, rlz, rnum, rdW = orc.tab_loss_grad(table, W, nf, lab, nl, 0)
    assert_loss_close(_np(loss), rl)
    assert_grad_marginal_close(_np(dW), rdW, table_den_marginals(orc, table, W, nf, lab, nl, 0),
                               rlz, rnum)

  def num_forward(lab, labd):
    assert_loss_close(_np(nat.table_num_forward(g, Wd, nfd, labd, nld, SID['Log'])),
                      orc.tab_num_forward(table, W, nf, lab, nl, 0))

  for lds_of_u, run in ((lambda u: str_grad_lds(u, 0, True), num_backward('MaxTropical', orc.MAX)),
                        (lambda u: str_grad_lds(u, 0, False), num_backward('Real', orc.REAL)),
                        (lambda u: loss_grad_lds_n(u, 0), loss_grad),
                        (num_fwd_lds, num_forward)):
    U0 = _first_refused(lds_of_u)
    for U in (U0, U0 - 1, U0 - 2):
      lab = rng.integers(1, 4, (B, U)).astype(np.int32)
      labd = torch.tensor(lab).to(cuda)
      if U == U0:
        with pytest.raises(nat.LatticeLibraryError, match=unsupported):
          run(lab, labd)
      elif U == U0 - 1:
        try:
          run(lab, labd)
        except nat.LatticeLibraryError as e:
          assert re.search(unsupported, str(e)), e
      else:
        run(lab, labd)
  # lt_table_num_backward's refusal is in its workspace query too
  lab = torch.tensor(rng.integers(1, 4, (B, _first_refused(lambda u: str_grad_lds(u, 0, True))))
                     .astype(np.int32)).to(cuda)
  with pytest.raises(nat.LatticeLibraryError, match=unsupported):
    nat.table_num_backward_check(g, Wd, lab, SID['MaxTropical'])
