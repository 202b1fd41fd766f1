"""The chunked scan (lt_chunk.hip) at every chunk length its LDS budget admits
at V = 32: L = 8, 7, 6, 6, 5 for U = 5, 30, 60, 100, 110 (both
positions-per-lane classes: NPG <= 64 and NPG > 64), fp32 and bf16, at
T = 2 L + 1: three chunks, one live frame in the last. A ragged case puts
num_frames on 0, 1, L, L + 1 and T; one V = 16 case runs the run-time-stride
kernels.

Every case runs lt_loss_grad with design = DESIGN_CHUNK on a NaN-poisoned
workspace against the C oracle under the parity suite's bounds
(golden_cases.assert_loss_close / assert_grad_marginal_close), asserts that
no utterance left the chunked kernels for the frame-serial fallback, and
that a second call returns the same bits.

ck_marg_kernel is instantiated per chunk length for fp32 W at V = 32
(LT_CK_GEOM). test_specialised_and_generic_same_bits runs every case above
through that instantiation and through the run-time-geometry kernel
(LT_CHUNK_GENERIC=1, which the diagnostic build reads per call), demands
bit-equal loss, log_z, num and dW, and checks which kernel each call
launched (the planned L for fp32 at V = 32, the run-time kernel otherwise).
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

N = 1  # bigram: the chunked design's only context size
# U -> the chunk length at V = 32 (ck_plan's LDS budget; bench.py's chunk_len mirrors it)
CHUNK_LEN = {5: 8, 30: 7, 60: 6, 100: 6, 110: 5}


def _orc():
  from oracle import oracle as orc  # test infrastructure only
  return orc


def _problem(B, T, U, V, seed, nf=None):
  """Utterance 0 full length, the rest random (or `nf`); labels with
  epsilons; every string reachable (a label needs a frame)."""
  rng = np.random.default_rng(seed)
  W = rng.standard_normal((B, T, V + 1, V + 1)).astype(np.float32)
  if nf is None:
    nf = rng.integers(0, T + 1, B).astype(np.int32)
    nf[0] = T
  nf = np.asarray(nf, np.int32)
  lab = rng.integers(0, V + 1, (B, U)).astype(np.int32)
  nl = rng.integers(0, U + 1, B).astype(np.int32)
  nl[0] = U
  return W, nf, lab, np.minimum(nl, nf).astype(np.int32)


def _poisoned_ws(W, V, U, local):
  nb = nat.loss_grad_workspace_bytes(W, V, N, U, local, nat.DESIGN_CHUNK)
  return torch.full([max(nb, 1)], 0xFF, dtype=torch.uint8, device=W.device)


def _check(cuda, W, nf, lab, nl, V, bf16):
  orc = _orc()
  if bf16:
    W = torch.tensor(W).bfloat16().float().numpy()
  B, U = W.shape[0], lab.shape[1]
  Wd = torch.tensor(W).to(torch.bfloat16 if bf16 else torch.float32).to(cuda)
  nfd, labd, nld = (torch.tensor(x).to(cuda) for x in (nf, lab, nl))
  for local in (False, True):
    ws = _poisoned_ws(Wd, V, U, local)
    loss, lz, num, dW = nat.loss_grad(Wd, nfd, labd, nld, V, N, local, workspace=ws,
                                      design=nat.DESIGN_CHUNK)
    torch.cuda.synchronize()
    rl, rlz, rnum, rdW = orc.loss_grad(W, nf, lab, nl, V, N, local_norm=local)
    den = None if local else orc.den_grad(W, nf, V, N)[1]
    assert_loss_close(loss.cpu().numpy(), rl)
    assert_grad_marginal_close(dW.float().cpu().numpy(), rdW, den, rlz, rnum, bf16)
    assert nat.chunk_fallback_count(ws, B) == 0
    ws2 = _poisoned_ws(Wd, V, U, local)
    loss2, lz2, num2, dW2 = nat.loss_grad(Wd, nfd, labd, nld, V, N, local, workspace=ws2,
                                          design=nat.DESIGN_CHUNK)
    assert torch.equal(loss, loss2) and torch.equal(dW, dW2)
    assert torch.equal(lz, lz2) and torch.equal(num, num2)


def _length_case(U, bf16):
  L = CHUNK_LEN[U]
  W, nf, lab, nl = _problem(3, 2 * L + 1, U, 32, seed=1000 + U)
  return W, nf, lab, nl, 32, bf16


def _ragged_case(U):
  L = CHUNK_LEN[U]
  T = 2 * L + 1
  nf = [0, 1, L, L + 1, T]
  W, nf, lab, nl = _problem(len(nf), T, U, 32, seed=2000 + U, nf=nf)
  return W, nf, lab, nl, 32, False


def _v16_case():
  W, nf, lab, nl = _problem(3, 23, 30, 16, seed=3000)
  return W, nf, lab, nl, 16, False


def cases():
  """(name, (W, nf, lab, nl, V, bf16)) of every case of this file."""
  for U in sorted(CHUNK_LEN):
    for bf16 in (False, True):
      yield f'U={U} {"bf16" if bf16 else "f32"}', _length_case(U, bf16)
  for U in (30, 100):
    yield f'ragged U={U}', _ragged_case(U)
  yield 'V=16', _v16_case()


def test_chunk_len_table():
  """CHUNK_LEN against the mirror of ck_plan's LDS budget that bench.py keeps
  (the T of every case here is chosen from it)."""
  sys.path.insert(0, ROOT)
  import bench
  for U, L in CHUNK_LEN.items():
    assert bench.chunk_len(3, 2 * L + 1, U, 32) == L, U


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('U', sorted(CHUNK_LEN))
def test_chunk_lengths_vs_oracle(cuda, U, dt):
  W, nf, lab, nl, V, bf16 = _length_case(U, dt == 'bf16')
  _check(cuda, W, nf, lab, nl, V, bf16)


@pytest.mark.gpu
@pytest.mark.parametrize('U', [30, 100])
def test_chunk_lengths_ragged(cuda, U):
  """num_frames on 0, 1, L, L + 1 and T: an empty utterance, one frame,
  exactly one chunk, one frame into the second, and all three chunks."""
  W, nf, lab, nl, V, bf16 = _ragged_case(U)
  _check(cuda, W, nf, lab, nl, V, bf16)


@pytest.mark.gpu
def test_chunk_v16_runtime_strides(cuda):
  """V = 16: the kernels with run-time strides (FULL = false)."""
  W, nf, lab, nl, V, bf16 = _v16_case()
  _check(cuda, W, nf, lab, nl, V, bf16)


@pytest.mark.gpu
def test_specialised_and_generic_same_bits(cuda):
  """Every case through the per-length instantiation and through the
  run-time-geometry kernel: bit-equal loss, log_z, num and dW (one child
  process on the diagnostic build, tests/diag_geometry_child.py)."""
  env = dict(os.environ, LT_LIB_PATH=DIAG)
  env.pop('LT_CHUNK_GENERIC', None)
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'diag_geometry_child.py')],
                     env=env, capture_output=True, text=True, timeout=300)
  assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
  assert r.stdout.strip().endswith('ok'), r.stdout[-2000:]
  assert r.stdout.count('same bits:') == len(list(cases()))
