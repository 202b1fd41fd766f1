"""Phase C's exit (lt_chunk.hip, ck_marg_kernel from its last barrier on): the
chunk's dW leaves its LDS image by 16-byte granules, each thread's reads
issued before its stores where the chunk length is a compile-time constant
(fp32 W at V = 32), by a loop that reads two granules ahead otherwise; the
unaligned bytes in front of the first whole granule and behind the last go
out as single elements, and the padding frames behind the live ones as zeros.
What can go wrong is a granule dropped, written twice from the wrong place, or
written outside the chunk.

Every case compares loss and dW with the C oracle under the parity suite's
bounds (golden_cases.assert_loss_close / assert_grad_marginal_close), on
0xFF-filled outputs and workspaces (poisoned_buffers), through lt_loss_grad
and through lt_chunk_forward + lt_chunk_backward, and demands exact zeros in
every padding frame.

  * V = 32, fp32 and bf16, U = 5, 30, 60, 100, 120 (fp32: L = 8, 7, 6, 6, 5;
    one and two string positions a lane), T = 3 L + 1 or 3 L + 2 (odd, so that the
    utterances' first frames reach every offset), num_frames 0, 1, L - 1,
    L, L + 1, T, and behind them the utterances _cover() adds so that every
    chunk start offset within a granule (fp32: 0, 4, 8, 12; bf16: the even
    offsets 0 ... 14) meets every live-frame count 1 ... L.
    test_offsets_and_frame_counts_covered decides that on the CPU from the
    mirror of ck_plan (_plan_len).
  * The run-time kernels at V = 1, 2, 5, 16, 31, U = 1, 63, 100, B = 3,
    T = 2 L + 1: frames of 16 and 36 bytes (fp32) and 8 bytes (bf16), where a
    chunk can be shorter than one granule and the body is empty.
  * Guards: lt_loss_grad_ex with dW 128 bytes inside a larger 0xFF-filled
    allocation, fp32 and bf16: the 128 bytes in front and behind stay 0xFF.
  * A NaN utterance and an utterance that fails phase C's certificate (finite
    loss: at one frame alpha sits on one state and beta on another, and every
    arc between the two lies 100 nats below the rest, so the frame's total is
    far more than 2^64 below max alpha x max beta) beside ordinary utterances:
    exactly those two are flagged, and every utterance matches the oracle.
  * test_specialised_and_runtime_same_bits: a child process on the diagnostic
    build (tests/diag_dw_exit_child.py) runs every fp32 V = 32 case through the
    instantiation of its chunk length and through the run-time kernel
    (LT_CHUNK_GENERIC=1): loss, log_z, num and dW bit for bit.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from last_torch_amd import _native as nat
from golden_cases import assert_grad_marginal_close, assert_loss_close
from poisoned_buffers import poison_, poisoned

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG = os.path.join(ROOT, 'build', 'diag', 'liblt_lattice_diag.so')
N = 1
SPEC_US = (5, 30, 60, 100, 120)
SPEC_LEN = {5: 8, 30: 7, 60: 6, 100: 6, 120: 5}  # fp32 at V = 32
RT_VS = (1, 2, 5, 16, 31)
RT_US = (1, 63, 100)


def _orc():
  from oracle import oracle as orc  # test infrastructure only
  return orc


def _plan_len(U, V, bf16):
  """ck_plan's chunk length: the largest L <= 32 whose phase-C LDS carve fits
  40 KiB (never below 4); bench.chunk_len is the same carve for fp32."""
  es = 2 if bf16 else 4
  FR = (V + 1) * (V + 1)
  FB, NPG, CP = FR * es, (U + 2) & ~1, (V + 4) & ~3
  al16 = lambda x: (x + 15) & ~15

  def carve(L):
    n16 = (L * FB + 30) // 16
    return (((n16 + 63) // 64) * 1024 + 2 * al16(4 * L * CP) + 2 * al16(4 * L * NPG) +
            al16(8 * L * NPG) + al16(32 * L) + al16(8 * NPG + 4 * U) + al16(4 * L) + 1024 +
            al16(4 * (2 * L + 3)) + (al16(4 * L * ((FR + 3) & ~3)) if bf16 else 0))

  L = 32
  while L > 4 and carve(L) > 40 * 1024:
    L -= 1
  return L


def _chunks(b, nf, T, L, V, bf16):
  """(start byte offset within a granule, live frames) of utterance b's live
  chunks: chunk k starts at frame k L of utterance b, element (b T + k L) FR."""
  FB = (V + 1) * (V + 1) * (2 if bf16 else 4)
  nf = max(0, min(int(nf), T))
  return [(((b * T + k * L) * FB) % 16, min(L, nf - k * L)) for k in range((nf + L - 1) // L)]


def _cover(nf, T, L, V, bf16):
  """`nf` and the fewest further utterances (greedy, in order) after which every
  start offset has met every live-frame count 1 ... L."""
  step = 2 if bf16 else 4
  want = {(o, n) for o in range(0, 16, step) for n in range(1, L + 1)}
  nf = list(nf)
  have = set()
  for b, x in enumerate(nf):
    have.update(_chunks(b, x, T, L, V, bf16))
  while not want <= have:
    b = len(nf)
    best = max(range(1, T + 1), key=lambda x: (len(set(_chunks(b, x, T, L, V, bf16)) - have), -x))
    nf.append(best)
    have.update(_chunks(b, best, T, L, V, bf16))
    assert len(nf) < 200
  return np.array(nf, np.int32)


def _problem(nf, T, U, V, seed):
  """Labels in [0, V + 2] (epsilons and out-of-range values), num_labels
  ragged with 0 and U, never above the frames (a label needs a frame)."""
  rng = np.random.default_rng(seed)
  B = len(nf)
  W = rng.standard_normal((B, T, V + 1, V + 1)).astype(np.float32)
  lab = rng.integers(0, V + 3, (B, U)).astype(np.int32)
  nl = rng.integers(0, U + 1, B).astype(np.int32)
  nl[-1] = U
  return W, np.asarray(nf, np.int32), lab, np.minimum(nl, nf).astype(np.int32)


def _spec_case(U, bf16):
  L = _plan_len(U, 32, bf16)
  T = (3 * L + 1) | 1  # odd, so that the utterances' first frames reach every offset
  nf = _cover([0, 1, L - 1, L, L + 1, T], T, L, 32, bf16)
  return _problem(nf, T, U, 32, 9000 + 2 * U + bf16) + (32, bf16)


def _rt_case(V, U, bf16):
  L = _plan_len(U, V, bf16)
  T = 2 * L + 1
  return _problem([T, L + 1, 1], T, U, V, 9500 + 100 * V + 2 * U + bf16) + (V, bf16)


def spec_cases():
  for U in SPEC_US:
    for bf16 in (False, True):
      yield f'U={U} {"bf16" if bf16 else "f32"}', _spec_case(U, bf16)


_REF = {}


def _ref(key, W, nf, lab, nl, V, local):
  """The oracle's (loss, log_z, num, dW, den marginals), once per case."""
  k = (key, local)
  if k not in _REF:
    orc = _orc()
    rl, rlz, rnum, rdW = orc.loss_grad(W, nf, lab, nl, V, N, local_norm=local)
    den = None if local else orc.den_grad(W, nf, V, N)[1]
    for x in (rl, rlz, rnum, rdW) + (() if den is None else (den,)):
      x.setflags(write=False)
    _REF[k] = (rl, rlz, rnum, rdW, den)
  return _REF[k]


def _host(W, bf16):
  return torch.tensor(W).bfloat16().float().numpy() if bf16 else W


def _dev(cuda, W, nf, lab, nl, bf16):
  Wd = torch.tensor(W).to(torch.bfloat16 if bf16 else torch.float32).to(cuda)
  return (Wd,) + tuple(torch.tensor(x).to(cuda) for x in (nf, lab, nl))


def _poisoned_ws(Wd, V, U, local):
  nb = nat.loss_grad_workspace_bytes(Wd, V, N, U, local, nat.DESIGN_CHUNK)
  return torch.full([max(nb, 1)], 0xFF, dtype=torch.uint8, device=Wd.device)


def _assert_close(loss, dW, ref, bf16, rows=None):
  rl, rlz, rnum, rdW, den = ref
  s = slice(None) if rows is None else rows
  assert_loss_close(loss.cpu().numpy()[s], rl[s])
  assert_grad_marginal_close(dW.float().cpu().numpy()[s], rdW[s], None if den is None else den[s],
                             rlz[s], rnum[s], bf16)


def _assert_padding_zero(dW, nf):
  """Padding frames and padding chunks: exact zeros (0xFF bytes are NaN)."""
  d = dW.float().cpu().numpy()
  for b, x in enumerate(nf):
    pad = d[b, max(int(x), 0):]
    assert not pad.any() and not np.isnan(pad).any(), (b, int(x))


def _check(cuda, key, W, nf, lab, nl, V, bf16, locals_=(False, True)):
  W = _host(W, bf16)
  d = _dev(cuda, W, nf, lab, nl, bf16)
  U = lab.shape[1]
  for local in locals_:
    ref = _ref(key, W, nf, lab, nl, V, local)
    ws = _poisoned_ws(d[0], V, U, local)
    with poisoned(nat):
      loss, _, _, dW = nat.loss_grad(*d, V, N, local, workspace=ws, design=nat.DESIGN_CHUNK)
      torch.cuda.synchronize()
      assert nat.chunk_fallback_count(ws, len(nf)) == 0
      _assert_close(loss, dW, ref, bf16)
      _assert_padding_zero(dW, nf)
      loss2, _, _, state = nat.chunk_forward(*d, V, N, local)
      dW2 = nat.chunk_backward(*d, V, N, local, state)
      torch.cuda.synchronize()
    _assert_close(loss2, dW2, ref, bf16)
    _assert_padding_zero(dW2, nf)


def test_chunk_lengths():
  """SPEC_LEN against the mirrors of ck_plan's LDS budget (this file's, which
  knows bf16, and bench.py's)."""
  sys.path.insert(0, ROOT)
  import bench
  for U, L in SPEC_LEN.items():
    assert _plan_len(U, 32, False) == L == bench.chunk_len(4, 3 * L + 1, U, 32), U
  for V in RT_VS:
    for U in RT_US:
      assert _plan_len(U, V, False) == bench.chunk_len(3, 65, U, V), (V, U)


def test_offsets_and_frame_counts_covered():
  """Every chunk start offset within a 16-byte granule meets every live-frame
  count 1 ... L, at every chunk length, in the V = 32 cases (decided here from
  the plan's mirror, not on the GPU)."""
  seen_len = set()
  for name, (W, nf, lab, nl, V, bf16) in spec_cases():
    U = lab.shape[1]
    L, T = _plan_len(U, V, bf16), W.shape[1]
    have = set()
    for b, x in enumerate(nf):
      have.update(_chunks(b, x, T, L, V, bf16))
    for o in range(0, 16, 2 if bf16 else 4):
      for n in range(1, L + 1):
        assert (o, n) in have, (name, o, n)
    if not bf16:
      assert {o for o, _ in have} == {0, 4, 8, 12}, name
      seen_len.add(L)
    assert len(nf) <= 80, (name, len(nf))  # the cases stay small
  assert seen_len == {5, 6, 7, 8}


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('U', SPEC_US)
def test_every_offset_and_frame_count(cuda, U, dt):
  bf16 = dt == 'bf16'
  W, nf, lab, nl, V, _ = _spec_case(U, bf16)
  _check(cuda, ('spec', U, dt), W, nf, lab, nl, V, bf16)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('U', RT_US)
@pytest.mark.parametrize('V', RT_VS)
def test_runtime_kernels_small_frames(cuda, V, U, dt):
  bf16 = dt == 'bf16'
  W, nf, lab, nl, V, _ = _rt_case(V, U, bf16)
  _check(cuda, ('rt', V, U, dt), W, nf, lab, nl, V, bf16, locals_=(False,))


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_nothing_written_outside_dw(cuda, dt):
  """lt_loss_grad_ex with dW 128 bytes inside a larger 0xFF-filled allocation:
  the bytes in front and behind are untouched, dW matches the oracle."""
  bf16 = dt == 'bf16'
  U = 100
  W, nf, lab, nl, V, _ = _spec_case(U, bf16)
  W = _host(W, bf16)
  Wd, nfd, labd, nld = _dev(cuda, W, nf, lab, nl, bf16)
  B = len(nf)
  nbytes = Wd.numel() * Wd.element_size()
  G = 128
  buf = torch.full([nbytes + 2 * G], 0xFF, dtype=torch.uint8, device=cuda)
  assert buf.data_ptr() % 16 == 0
  ws = _poisoned_ws(Wd, V, U, False)
  loss, lz, num = (poison_(torch.empty([B], device=cuda)) for _ in range(3))
  pb = nat._problem(Wd, V, N, U)
  nat._check(nat.lib().lt_loss_grad_ex(
      ctypes.byref(pb), 0, nat.DESIGN_CHUNK, nat._ptr(Wd), nat._ptr(nfd), nat._ptr(labd),
      nat._ptr(nld), nat._ptr(loss), nat._ptr(lz), nat._ptr(num),
      ctypes.c_void_p(buf.data_ptr() + G), nat._ptr(ws), ws.numel(), nat._stream()),
      'lt_loss_grad_ex')
  torch.cuda.synchronize()
  assert bool((buf[:G] == 0xFF).all()) and bool((buf[G + nbytes:] == 0xFF).all())
  dW = buf[G:G + nbytes].view(Wd.dtype).view(Wd.shape)
  _assert_close(loss, dW, _ref(('spec', U, dt), W, nf, lab, nl, V, False), bf16)
  _assert_padding_zero(dW, nf)


def _fallback_case():
  """B = 5 at U = 100 (L = 6), T = 3 L + 1: utterance 1 holds a NaN, utterance
  3 fails the certificate at a frame of its second chunk."""
  U, V = 100, 32
  L = SPEC_LEN[U]
  T = 3 * L + 1
  rng = np.random.default_rng(9900)
  B = 5
  W = rng.standard_normal((B, T, V + 1, V + 1)).astype(np.float32)
  nf = np.array([T, T, T - 2, T, L + 1], np.int32)
  lab = rng.integers(1, V + 1, (B, U)).astype(np.int32)
  nl = np.array([T // 2, 5, 0, 4, 3], np.int32)
  W[1, 2 * L + 1, 3, 4] = np.nan
  f, s1, s2 = L + 2, 3, 7
  W[3, f - 1] = -100.0
  W[3, f - 1, :, s1] = 0.0  # alpha_f sits on state s1
  W[3, f + 1] = -100.0
  W[3, f + 1, s2, :] = 0.0  # beta_{f+1} sits on state s2
  W[3, f] = 0.0
  W[3, f, s1, s2] = -100.0  # and the one arc from s1 to s2 is far below the rest
  return W, nf, lab, nl, V, {1, 3}


@pytest.mark.gpu
def test_fallback_beside_fast_path(cuda):
  W, nf, lab, nl, V, flagged = _fallback_case()
  d = _dev(cuda, W, nf, lab, nl, False)
  U, B = lab.shape[1], len(nf)
  ref = _ref('fallback', W, nf, lab, nl, V, False)
  fin = [b for b in range(B) if np.isfinite(ref[0][b])]
  assert 3 in fin and 1 not in fin  # the certificate case has a finite loss
  ws = _poisoned_ws(d[0], V, U, False)
  with poisoned(nat):
    loss, _, _, dW = nat.loss_grad(*d, V, N, False, workspace=ws, design=nat.DESIGN_CHUNK)
    torch.cuda.synchronize()
    got = set(np.flatnonzero(ws[:4 * B].view(torch.int32).cpu().numpy()).tolist())
    assert got == flagged, got
    _assert_close(loss, dW, ref, False, rows=fin)
    assert_loss_close(loss.cpu().numpy(), ref[0])
    _assert_padding_zero(dW[fin], nf[fin])
    loss2, _, _, state = nat.chunk_forward(*d, V, N, False)
    dW2 = nat.chunk_backward(*d, V, N, False, state)
    torch.cuda.synchronize()
  _assert_close(loss2, dW2, ref, False, rows=fin)
  assert_loss_close(loss2.cpu().numpy(), ref[0])
  _assert_padding_zero(dW2[fin], nf[fin])


@pytest.mark.gpu
def test_specialised_and_runtime_same_bits(cuda):
  """tests/diag_dw_exit_child.py on the diagnostic build."""
  env = dict(os.environ, LT_LIB_PATH=DIAG)
  env.pop('LT_CHUNK_GENERIC', None)
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'diag_dw_exit_child.py')],
                     env=env, capture_output=True, text=True, timeout=300)
  assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
  assert r.stdout.strip().endswith('ok'), r.stdout[-2000:]
  assert r.stdout.count('same bits:') == len(SPEC_US) + 1
