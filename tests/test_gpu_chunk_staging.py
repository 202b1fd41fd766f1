"""The heads of the chunked scan's workgroups (lt_chunk.hip): phase C's wave 0
issues the walks' progress words, the chunk's frame offsets and the
utterance's gather tables (written once per utterance by its walks to the
state) ahead of the chunk's W and waits for them with a counted vmcnt. A
wrong count, stale or misplaced tables or a misplaced barrier shows as foreign
gather offsets, frame offsets or boundary values, so every
case here runs against the C oracle under the parity suite's bounds
(golden_cases.assert_loss_close / assert_grad_marginal_close), on NaN-poisoned
or stale workspaces (the state's table region included: every workspace byte
is poisoned or left over from another problem).

Shapes (V = 32 unless said; L = the plan's chunk length for the shape,
_plan_len mirrors ck_plan):
  * T = 3 L + 1 with num_frames in {0, 1, L - 1, L, L + 1, T}: chunks of 1,
    L - 1 and L live frames (the number of W DMA instructions behind the
    counted wait differs), an empty utterance, one frame, padding chunks;
  * U in {1, 63, 64, 65, 127}: both positions-per-lane classes; 4 U is no
    multiple of 16 for four of them, so utterance b's labels start at every
    shift 0, 4, 8, 12 within a 16-byte granule (and one case passes a label
    tensor that itself starts 4 bytes past a granule), while its tables start
    on one;
  * num_labels ragged with 0; labels hold 0 (epsilon) and values above V;
  * fp32 and bf16 (a bf16 frame is no multiple of 16 bytes); V = 16 runs the
    run-time-geometry kernels;
  * global and local normalisation (local: no den progress words);
  * lt_loss_grad (the walks finish in phase C's launch, which polls them) and
    lt_chunk_forward + lt_chunk_backward (no poll, the tables from the state
    of another call); B above the device's CU
    count (the unfused route: ck_combine_kernel), and LT_CHUNK_FUSE=0 at B = 3
    in a child process on the diagnostic build, which reads it per call;
  * two calls on different problems through one workspace and one set of
    outputs (poisoned_buffers.stale), the second compared in full;
  * a masked-arc utterance (chunk flag 3) beside a NaN utterance (flag 2):
    only the NaN utterance leaves for the frame-serial kernels;
  * a captured graph replayed on new W and new labels against eager calls.
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
from poisoned_buffers import poisoned, stale

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG = os.path.join(ROOT, 'build', 'diag', 'liblt_lattice_diag.so')
N = 1
US = (1, 63, 64, 65, 127)


def _orc():
  from oracle import oracle as orc  # test infrastructure only
  return orc


def _plan_len(U, V, bf16):
  """ck_plan's chunk length: the largest L <= 32 whose phase-C LDS carve fits
  40 KiB (never below 4)."""
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


def test_plan_len_mirror():
  """_plan_len against bench.py's mirror of the same carve (fp32)."""
  sys.path.insert(0, ROOT)
  import bench
  for U in US + (5, 30, 100):
    for V in (16, 32):
      assert _plan_len(U, V, False) == bench.chunk_len(3, 100, U, V), (U, V)


def _ragged(U, V, bf16, seed):
  """B = 6 at T = 3 L + 1: num_frames 0, 1, L - 1, L, L + 1, T; labels in
  [0, V + 2] (epsilons and out-of-range values); num_labels ragged with 0,
  never above the frames (a label needs a frame)."""
  L = _plan_len(U, V, bf16)
  T = 3 * L + 1
  nf = np.array([0, 1, L - 1, L, L + 1, T], np.int32)
  rng = np.random.default_rng(seed)
  W = rng.standard_normal((len(nf), T, V + 1, V + 1)).astype(np.float32)
  lab = rng.integers(0, V + 3, (len(nf), U)).astype(np.int32)
  nl = np.array([0, 1, U // 2, U, 0, U], np.int32)
  return W, nf, lab, np.minimum(nl, nf).astype(np.int32)


_REF = {}


def _ref(key, W, nf, lab, nl, V, local):
  """The oracle's (loss, log_z, num, dW, den marginals), computed once per case."""
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


def _assert_close(out, ref, bf16, rows=None):
  loss, _, _, dW = out
  rl, rlz, rnum, rdW, den = ref
  s = slice(None) if rows is None else rows
  assert_loss_close(loss.cpu().numpy()[s], rl[s])
  assert_grad_marginal_close(dW.float().cpu().numpy()[s], rdW[s], None if den is None else den[s],
                             rlz[s], rnum[s], bf16)


def _poisoned_ws(Wd, V, U, local):
  nb = nat.loss_grad_workspace_bytes(Wd, V, N, U, local, nat.DESIGN_CHUNK)
  return torch.full([max(nb, 1)], 0xFF, dtype=torch.uint8, device=Wd.device)


def _loss_grad(Wd, nfd, labd, nld, V, local):
  ws = _poisoned_ws(Wd, V, labd.shape[1], local)
  with poisoned(nat):
    out = nat.loss_grad(Wd, nfd, labd, nld, V, N, local, workspace=ws, design=nat.DESIGN_CHUNK)
  torch.cuda.synchronize()
  return out, ws


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('U', US)
def test_ragged_frames_and_strings(cuda, U, dt):
  bf16 = dt == 'bf16'
  W, nf, lab, nl = _ragged(U, 32, bf16, seed=4000 + U)
  W = _host(W, bf16)
  Wd, nfd, labd, nld = _dev(cuda, W, nf, lab, nl, bf16)
  for local in (False, True):
    out, ws = _loss_grad(Wd, nfd, labd, nld, 32, local)
    _assert_close(out, _ref(('ragged', U, dt), W, nf, lab, nl, 32, local), bf16)
    assert nat.chunk_fallback_count(ws, len(nf)) == 0


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_v16_runtime_geometry(cuda, dt):
  bf16 = dt == 'bf16'
  W, nf, lab, nl = _ragged(63, 16, bf16, seed=4500)
  W = _host(W, bf16)
  Wd, nfd, labd, nld = _dev(cuda, W, nf, lab, nl, bf16)
  for local in (False, True):
    out, ws = _loss_grad(Wd, nfd, labd, nld, 16, local)
    _assert_close(out, _ref(('v16', dt), W, nf, lab, nl, 16, local), bf16)
    assert nat.chunk_fallback_count(ws, len(nf)) == 0


@pytest.mark.gpu
def test_labels_off_granule(cuda):
  """The label tensor itself starts 4 bytes past a 16-byte granule."""
  U = 63
  W, nf, lab, nl = _ragged(U, 32, False, seed=4000 + U)
  Wd, nfd, labd, nld = _dev(cuda, W, nf, lab, nl, False)
  flat = torch.full([labd.numel() + 8], -7, dtype=torch.int32, device=cuda)
  view = flat[1:1 + labd.numel()].view(labd.shape)
  view.copy_(labd)
  assert view.data_ptr() % 16 == 4 and view.is_contiguous()
  out, ws = _loss_grad(Wd, nfd, view, nld, 32, False)
  _assert_close(out, _ref(('ragged', U, 'f32'), W, nf, lab, nl, 32, False), False)
  assert nat.chunk_fallback_count(ws, len(nf)) == 0


def _pair(d, V, local):
  loss, lz, num, state = nat.chunk_forward(*d, V, N, local)
  return loss, lz, num, nat.chunk_backward(*d, V, N, local, state)


@pytest.mark.gpu
@pytest.mark.parametrize('U,V,dt', [(63, 32, 'f32'), (127, 32, 'bf16'), (63, 16, 'f32')])
def test_forward_backward_pair(cuda, U, V, dt):
  """lt_chunk_forward + lt_chunk_backward: phase C without the poll, the
  state handed from one call to the next."""
  bf16 = dt == 'bf16'
  W, nf, lab, nl = _ragged(U, V, bf16, seed=4500 if V == 16 else 4000 + U)
  W = _host(W, bf16)
  key = ('v16', dt) if V == 16 else ('ragged', U, dt)
  Wd, nfd, labd, nld = _dev(cuda, W, nf, lab, nl, bf16)
  for local in (False, True):
    with poisoned(nat):
      out = _pair((Wd, nfd, labd, nld), V, local)
    torch.cuda.synchronize()
    _assert_close(out, _ref(key, W, nf, lab, nl, V, local), bf16)


@pytest.mark.gpu
def test_unfused_route_above_cu_count(cuda):
  """B one above the CU count: ck_combine_kernel walks after phase A's
  launch, and phase C's launch still finishes and polls the walks."""
  V, U = 32, 5
  L = _plan_len(U, V, False)
  T = 2 * L + 1
  B = torch.cuda.get_device_properties(cuda).multi_processor_count + 1
  rng = np.random.default_rng(4600)
  W = rng.standard_normal((B, T, V + 1, V + 1)).astype(np.float32)
  nf = rng.integers(0, T + 1, B).astype(np.int32)
  nf[:3] = (T, L, 1)
  lab = rng.integers(0, V + 3, (B, U)).astype(np.int32)
  nl = np.minimum(rng.integers(0, U + 1, B), nf).astype(np.int32)
  Wd, nfd, labd, nld = _dev(cuda, W, nf, lab, nl, False)
  out, ws = _loss_grad(Wd, nfd, labd, nld, V, False)
  _assert_close(out, _ref('unfused', W, nf, lab, nl, V, False), False)
  assert nat.chunk_fallback_count(ws, B) == 0


@pytest.mark.gpu
def test_unfused_route_small_batch_child(cuda):
  """LT_CHUNK_FUSE=0 at B = 3 (the diagnostic build reads it per call):
  tests/diag_staging_child.py."""
  env = dict(os.environ, LT_LIB_PATH=DIAG, LT_CHUNK_FUSE='0')
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'diag_staging_child.py')],
                     env=env, capture_output=True, text=True, timeout=300)
  assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
  assert r.stdout.strip().endswith('ok'), r.stdout[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_second_problem_through_stale_buffers(cuda, dt):
  """Two calls on different problems of one shape through the same outputs
  and workspace: the second finds the first's tables, frame offsets, flags and
  tags, and must match the oracle in full."""
  bf16 = dt == 'bf16'
  U = 65
  W1, nf1, lab1, nl1 = _ragged(U, 32, bf16, seed=4700)
  W2, nf2, lab2, nl2 = _ragged(U, 32, bf16, seed=4000 + U)
  nf1, nl1 = nf1[::-1].copy(), np.minimum(nl1[::-1], nf1[::-1]).astype(np.int32)
  W2 = _host(W2, bf16)
  d1 = _dev(cuda, W1, nf1, lab1, nl1, bf16)
  d2 = _dev(cuda, W2, nf2, lab2, nl2, bf16)
  for local in (False, True):
    with stale(nat) as s:
      s.record(nat.loss_grad, *d1, 32, N, local, design=nat.DESIGN_CHUNK)
      out = s.replay(nat.loss_grad, *d2, 32, N, local, design=nat.DESIGN_CHUNK)
      torch.cuda.synchronize()
      _assert_close(out, _ref(('ragged', U, dt), W2, nf2, lab2, nl2, 32, local), bf16)
    with stale(nat) as s:
      s.record(_pair, d1, 32, local)
      out = s.replay(_pair, d2, 32, local)
      torch.cuda.synchronize()
      _assert_close(out, _ref(('ragged', U, dt), W2, nf2, lab2, nl2, 32, local), bf16)


@pytest.mark.gpu
def test_masked_and_nan_utterances(cuda):
  """A masked (-inf) arc (chunk flag 3: stays on the chunked path under phase
  C's certificate) beside a NaN weight (flag 2: the frame-serial kernels) and
  an ordinary utterance: only the NaN utterance is flagged; the finite ones
  match the oracle, the NaN one has the oracle's NaN loss."""
  V, U = 32, 30
  L = _plan_len(U, V, False)
  T = 3 * L + 1
  rng = np.random.default_rng(4800)
  W = rng.standard_normal((3, T, V + 1, V + 1)).astype(np.float32)
  W[0, L + 2, 5, 7] = -np.inf
  W[1, 2 * L + 1, 3, 4] = np.nan
  nf = np.array([T, T, T - 2], np.int32)
  lab = rng.integers(1, V + 1, (3, U)).astype(np.int32)
  nl = np.array([T // 2, 5, 0], np.int32)
  Wd, nfd, labd, nld = _dev(cuda, W, nf, lab, nl, False)
  out, ws = _loss_grad(Wd, nfd, labd, nld, V, False)
  ref = _ref('masked_nan', W, nf, lab, nl, V, False)
  flags = ws[:12].view(torch.int32).cpu().numpy()
  assert (flags != 0).tolist() == [False, True, False], flags
  _assert_close(out, ref, False, rows=[0, 2])
  assert np.isnan(ref[0][1]) and bool(torch.isnan(out[0][1]))


@pytest.mark.gpu
def test_graph_replays_with_new_weights_and_labels(cuda):
  """The hand-off words, which phase C's head now reads before its W: a
  captured lt_loss_grad replayed on new W and new labels gives an eager
  call's bits."""
  V, U, B, T = 32, 63, 20, 100

  def inputs(seed):
    g = torch.Generator(device=cuda)
    g.manual_seed(seed)
    W = torch.randn([B, T, V + 1, V + 1], generator=g, device=cuda)
    lab = torch.randint(0, V + 3, [B, U], generator=g, device=cuda, dtype=torch.int32)
    return W, lab

  g0 = torch.Generator(device=cuda)
  g0.manual_seed(11)
  nf = torch.randint(T // 2, T + 1, [B], generator=g0, device=cuda, dtype=torch.int32)
  nl = torch.randint(0, T // 2, [B], generator=g0, device=cuda, dtype=torch.int32).clamp(max=U)
  W, lab = inputs(1)
  pb = nat._problem(W, V, N, U)
  nbytes = nat.loss_grad_workspace_bytes(W, V, N, U, False, nat.DESIGN_CHUNK)
  ws = torch.full([max(nbytes, 1)], 0xFF, dtype=torch.uint8, device=cuda)
  loss, lz, num = (torch.empty([B], device=cuda) for _ in range(3))
  dW = torch.empty_like(W)

  def call():
    nat._check(nat.lib().lt_loss_grad_ex(
        ctypes.byref(pb), 0, nat.DESIGN_CHUNK, nat._ptr(W), nat._ptr(nf), nat._ptr(lab),
        nat._ptr(nl), nat._ptr(loss), nat._ptr(lz), nat._ptr(num), nat._ptr(dW), nat._ptr(ws),
        ws.numel(), nat._stream()), 'lt_loss_grad_ex')

  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(s):
    call()
  torch.cuda.current_stream().wait_stream(s)
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    call()
  for seed in (2, 3):
    W2, lab2 = inputs(seed)
    W.copy_(W2)
    lab.copy_(lab2)
    g.replay()
    torch.cuda.synchronize()
    rl, rlz, rnum, rdW = nat.loss_grad(W2, nf, lab2, nl, V, N, False, design=nat.DESIGN_CHUNK)
    torch.cuda.synchronize()
    assert torch.equal(loss, rl) and torch.equal(lz, rlz) and torch.equal(num, rnum), seed
    assert torch.equal(dW, rdW), (seed, float((dW - rdW).abs().max()))
  assert nat.chunk_fallback_count(ws, B) == 0
