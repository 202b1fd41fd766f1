"""Phase A of the chunked scan (lt_chunk.hip, transfer_role) in its
specialised form for fp32 W at V = 32: the frame geometry and the frame's
position in the chunk are compile-time constants there, one copy of the step
per position behind an `f < nt` guard.

Every case runs lt_loss_grad with design = DESIGN_CHUNK on a 0xFF-filled
workspace against the C oracle under the parity suite's bounds
(golden_cases.assert_loss_close / assert_grad_marginal_close).

  * Every frame count of every chunk length: U = 5, 30, 60, 100, 110 give
    L = 8, 7, 6, 6, 5 (test_gpu_chunk_geometry.test_chunk_len_table pins the
    table). T = 2 L, num_frames = 0, L + 1, ..., 2 L: the second chunk has
    1 ... L live frames, so every guard is taken both ways, the last utterance
    is full length (the tensor's last frame goes through the DMA's last-granule
    clamp), U = 5 reaches the second band group (frame 7 at L = 8), U = 30 / 60
    have one string position a lane and U = 100 / 110 two. The same at
    T = 2 L + 1 (one more utterance, full length): with a 4,356-byte frame an
    utterance's first frame then starts at every 16-byte alignment (0, 4, 8,
    12). No utterance may fall back, and a second call gives the same bits.
  * The range flags at L = 6 (U = 100), B = 8, T = 13: one utterance a case
    gets NaN, +inf, -inf or a value 200 below the frame's max at each of the
    four kinds of place a lane reads (a core arc, the start row, the blank
    column, (0, 0)), or one frame all -inf; at its second chunk's first frame
    and at its last. NaN, +inf and the all -inf frame send exactly that
    utterance to the frame-serial kernels; -inf and far-below-max stay on the
    chunked path. Either way every utterance matches the oracle.
  * The strict range: lt_loss_grad takes a chunk that phase A marks as
    outside the strict range (a -inf or far-below-max weight) under phase C's
    certificate, so it cannot tell whether the mark was set. lt_chunk_forward
    (the loss alone) sends such an utterance to the frame-serial kernels, so
    every case above also runs it: no utterance flagged in the frame-count
    cases, exactly the poisoned one in every flag case, the loss against the
    oracle.
  * test_specialised_and_runtime_same_bits: one child process on the diagnostic
    build runs every case above with and without LT_CHUNK_GENERIC=1 (the
    run-time phase A and phase C): loss, log_z, num, dW and the flagged set
    bit for bit, and lt_diag_chunk_ab_spec() says which phase A ran (also for
    one bf16 and one V = 16 case, which have no specialised form).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from last_torch_amd import _native as nat
from golden_cases import assert_grad_marginal_close, assert_loss_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG = os.path.join(ROOT, 'build', 'diag', 'liblt_lattice_diag.so')

N, V = 1, 32
CHUNK_LEN = {5: 8, 30: 7, 60: 6, 100: 6, 110: 5}  # as test_gpu_chunk_geometry.CHUNK_LEN

# the flag cases: the places a lane reads (row p, column y) and the poisons
PLACES = {'core': (5, 7), 'start_row': (0, 9), 'blank_col': (4, 0), 'w00': (0, 0)}
POISONS = ('nan', '+inf', '-inf', 'far')
FLAG_U, FLAG_B, FLAG_T = 100, 8, 13
FLAG_L = CHUNK_LEN[FLAG_U]
FLAG_FRAMES = {'first': FLAG_L, 'last': 2 * FLAG_L - 1}  # of the second chunk
FLAG_KINDS = [f'{pl}:{po}' for pl in PLACES for po in POISONS] + ['frame:-inf']


def _orc():
  from oracle import oracle as orc  # test infrastructure only
  return orc


def _frames_case(U, odd):
  """num_frames 0, L + 1, ..., 2 L at T = 2 L (odd: and 2 L + 1 at T = 2 L + 1);
  labels with epsilons; every string reachable (a label needs a frame)."""
  L = CHUNK_LEN[U]
  T = 2 * L + (1 if odd else 0)
  nf = np.array([0] + list(range(L + 1, T + 1)), np.int32)
  B = len(nf)
  rng = np.random.default_rng(7000 + 2 * U + odd)
  W = rng.standard_normal((B, T, V + 1, V + 1)).astype(np.float32)
  lab = rng.integers(0, V + 1, (B, U)).astype(np.int32)
  nl = rng.integers(0, U + 1, B).astype(np.int32)
  nl[-1] = U
  return W, nf, lab, np.minimum(nl, nf).astype(np.int32)


_FLAG_BASE = {}


def _flag_base():
  """The clean flag problem (every utterance ordinary), made once."""
  if not _FLAG_BASE:
    rng = np.random.default_rng(7700)
    W = rng.standard_normal((FLAG_B, FLAG_T, V + 1, V + 1)).astype(np.float32)
    nf = np.array([FLAG_T] * 6 + [FLAG_T - 1, FLAG_L + 1], np.int32)
    lab = rng.integers(1, V + 1, (FLAG_B, FLAG_U)).astype(np.int32)
    nl = np.minimum(rng.integers(0, 6, FLAG_B), nf).astype(np.int32)
    for x in (W, nf, lab, nl):
      x.setflags(write=False)
    _FLAG_BASE['p'] = (W, nf, lab, nl)
  return _FLAG_BASE['p']


def _flag_case(kind, where):
  """(W, nf, lab, nl, b, flagged): utterance b poisoned at frame
  FLAG_FRAMES[where]; flagged: it must leave for the frame-serial kernels."""
  W, nf, lab, nl = _flag_base()
  W = W.copy()
  b = (FLAG_KINDS.index(kind) + (3 if where == 'last' else 0)) % 6  # a full-length utterance
  t = FLAG_FRAMES[where]
  place, poison = kind.split(':')
  if place == 'frame':
    W[b, t] = -np.inf
    return W, nf, lab, nl, b, True
  p, y = PLACES[place]
  W[b, t, p, y] = {'nan': np.nan, '+inf': np.inf, '-inf': -np.inf,
                   'far': W[b, t].max() - 200.0}[poison]
  return W, nf, lab, nl, b, poison in ('nan', '+inf')


def cases():
  """(name, W, nf, lab, nl, locals, flagged set or None) of every case of this
  file, for the child process."""
  for U in sorted(CHUNK_LEN):
    for odd in (0, 1):
      yield (f'frames U={U} T=2L+{odd}',) + _frames_case(U, odd) + ((False, True), None)
  for kind in FLAG_KINDS:
    for where in FLAG_FRAMES:
      W, nf, lab, nl, b, flagged = _flag_case(kind, where)
      yield f'flags {kind} {where}', W, nf, lab, nl, (False,), ({b} if flagged else set())


def poisoned_ws(Wd, U, local):
  nb = nat.loss_grad_workspace_bytes(Wd, Wd.shape[-1] - 1, N, U, local, nat.DESIGN_CHUNK)
  return torch.full([max(nb, 1)], 0xFF, dtype=torch.uint8, device=Wd.device)


def flagged_set(ws, B):
  return set(np.flatnonzero(ws[:4 * B].view(torch.int32).cpu().numpy()).tolist())


def run_strict(Wd, nfd, labd, nld, local):
  """lt_chunk_forward: (loss, log_z, num), the flagged set."""
  loss, lz, num, state = nat.chunk_forward(Wd, nfd, labd, nld, Wd.shape[-1] - 1, N, local)
  torch.cuda.synchronize()
  return (loss, lz, num), flagged_set(state, Wd.shape[0])


def _run(Wd, nfd, labd, nld, local):
  ws = poisoned_ws(Wd, labd.shape[1], local)
  out = nat.loss_grad(Wd, nfd, labd, nld, V, N, local, workspace=ws, design=nat.DESIGN_CHUNK)
  torch.cuda.synchronize()
  return out, flagged_set(ws, Wd.shape[0])


_REF = {}


def _ref(key, W, nf, lab, nl, local):
  """The oracle's (loss, log_z, num, dW, den marginals), once per key."""
  if (key, local) not in _REF:
    orc = _orc()
    rl, rlz, rnum, rdW = orc.loss_grad(W, nf, lab, nl, V, N, local_norm=local)
    den = None if local else orc.den_grad(W, nf, V, N)[1]
    for x in (rl, rlz, rnum, rdW) + (() if den is None else (den,)):
      x.setflags(write=False)
    _REF[(key, local)] = (rl, rlz, rnum, rdW, den)
  return _REF[(key, local)]


def _assert_close(out, ref, rows):
  loss, _, _, dW = out
  rl, rlz, rnum, rdW, den = ref
  assert_loss_close(loss.cpu().numpy()[rows], rl[rows])
  assert_grad_marginal_close(dW.cpu().numpy()[rows], rdW[rows], None if den is None else den[rows],
                             rlz[rows], rnum[rows])


@pytest.mark.gpu
@pytest.mark.parametrize('odd', [0, 1])
@pytest.mark.parametrize('U', sorted(CHUNK_LEN))
def test_every_frame_count(cuda, U, odd):
  W, nf, lab, nl = _frames_case(U, odd)
  Wd, nfd, labd, nld = (torch.tensor(x).to(cuda) for x in (W, nf, lab, nl))
  rows = list(range(len(nf)))
  for local in (False, True):
    out, flagged = _run(Wd, nfd, labd, nld, local)
    _assert_close(out, _ref(('frames', U, odd), W, nf, lab, nl, local), rows)
    assert flagged == set()
    out2, flagged2 = _run(Wd, nfd, labd, nld, local)
    assert flagged2 == set()
    for x, y in zip(out, out2):
      assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    fwd, strict = run_strict(Wd, nfd, labd, nld, local)
    assert strict == set()
    assert_loss_close(fwd[0].cpu().numpy(), _ref(('frames', U, odd), W, nf, lab, nl, local)[0])


@pytest.mark.gpu
@pytest.mark.parametrize('where', sorted(FLAG_FRAMES))
@pytest.mark.parametrize('kind', FLAG_KINDS)
def test_range_flags(cuda, kind, where):
  W, nf, lab, nl, b, flagged = _flag_case(kind, where)
  Wd, nfd, labd, nld = (torch.tensor(x).to(cuda) for x in (W, nf, lab, nl))
  out, got = _run(Wd, nfd, labd, nld, False)
  assert got == ({b} if flagged else set()), (got, b, flagged)
  # the clean utterances against the clean problem's reference (an utterance's
  # results depend on its own inputs alone), the poisoned one against its own
  clean = [x for x in range(FLAG_B) if x != b]
  _assert_close(out, _ref('flags', *_flag_base(), False), clean)
  orc = _orc()
  one = slice(b, b + 1)
  rl, rlz, rnum, rdW = orc.loss_grad(W[one], nf[one], lab[one], nl[one], V, N, local_norm=False)
  loss = out[0].cpu().numpy()[one]
  if np.isfinite(rl[0]):
    den = orc.den_grad(W[one], nf[one], V, N)[1]
    assert_loss_close(loss, rl)
    assert_grad_marginal_close(out[3].cpu().numpy()[one], rdW, den, rlz, rnum)
  else:  # the oracle's NaN or infinity
    np.testing.assert_array_equal(loss, rl)
  # the strict range: every one of these poisons leaves it
  fwd, strict = run_strict(Wd, nfd, labd, nld, False)
  assert strict == {b}, (strict, b)
  l3 = fwd[0].cpu().numpy()
  assert_loss_close(l3[clean], _ref('flags', *_flag_base(), False)[0][clean])
  if np.isfinite(rl[0]):
    assert_loss_close(l3[one], rl)
  else:
    np.testing.assert_array_equal(l3[one], rl)


@pytest.mark.gpu
def test_specialised_and_runtime_same_bits(cuda):
  """tests/diag_phase_a_child.py on the diagnostic build."""
  env = dict(os.environ, LT_LIB_PATH=DIAG)
  env.pop('LT_CHUNK_GENERIC', None)
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'diag_phase_a_child.py')],
                     env=env, capture_output=True, text=True, timeout=300)
  assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
  assert r.stdout.strip().endswith('ok'), r.stdout[-2000:]
  assert r.stdout.count('same bits:') == len(list(cases())) + 2
