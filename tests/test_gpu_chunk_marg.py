"""Phase C of the chunked scan (lt_chunk.hip, ck_marg_kernel) at the smallest
shapes where its marginal path can go wrong: the numerator terms formed by
the numerator waves ahead of the den bits, the den pass by columns 1..V plus
the blank column, and the shift-mapped numerator-arc gather.

Every case runs lt_loss_grad with design = DESIGN_CHUNK on a NaN-poisoned
workspace, against the C oracle under the parity suite's bounds
(golden_cases.assert_loss_close / assert_grad_marginal_close), asserts that
no utterance left the chunked kernels for the frame-serial fallback, and
that a second call returns the same bits.
"""
import numpy as np
import pytest
import torch

import last_torch_amd as lt
from last_torch_amd import _native as nat
from golden_cases import assert_grad_marginal_close, assert_loss_close

pytestmark = pytest.mark.gpu

N = 1  # bigram: the chunked design's only context size


def _orc():
  from oracle import oracle as orc  # test infrastructure only
  return orc


def _random_problem(B, T, U, V, seed):
  """Full-length utterance 0, the rest of random length, labels with
  epsilons (as test_gpu_parity._random_problem)."""
  rng = np.random.default_rng(seed)
  W = rng.standard_normal((B, T, V + 1, V + 1)).astype(np.float32)
  nf = rng.integers(0, T + 1, B).astype(np.int32)
  nf[0] = T
  lab = rng.integers(0, V + 1, (B, U)).astype(np.int32)
  nl = rng.integers(0, U + 1, B).astype(np.int32)
  nl[0] = min(U, T)
  return W, nf, lab, nl


def _poisoned_ws(W, V, U, local):
  nb = nat.loss_grad_workspace_bytes(W, V, N, U, local, nat.DESIGN_CHUNK)
  return torch.full([max(nb, 1)], 0xFF, dtype=torch.uint8, device=W.device)


def _check(cuda, W, nf, lab, nl, V, bf16, locals_=(False, True)):
  orc = _orc()
  if bf16:
    W = torch.tensor(W).bfloat16().float().numpy()
  U = lab.shape[1]
  Wd = torch.tensor(W).to(torch.bfloat16 if bf16 else torch.float32).to(cuda)
  nfd, labd, nld = (torch.tensor(x).to(cuda) for x in (nf, lab, nl))
  B = W.shape[0]
  for local in locals_:
    ws = _poisoned_ws(Wd, V, U, local)
    loss, lz, _, dW = nat.loss_grad(Wd, nfd, labd, nld, V, N, local, workspace=ws,
                                    design=nat.DESIGN_CHUNK)
    torch.cuda.synchronize()
    rl, rlz, rnum, rdW = orc.loss_grad(W, nf, lab, nl, V, N, local_norm=local)
    den = None if local else orc.den_grad(W, nf, V, N)[1]
    assert_loss_close(loss.cpu().numpy(), rl)
    assert_grad_marginal_close(dW.float().cpu().numpy(), rdW, den, rlz, rnum, bf16)
    # the chunked kernels, not the frame-serial fallback, produced it
    assert nat.chunk_fallback_count(ws, B) == 0
    ws2 = _poisoned_ws(Wd, V, U, local)
    loss2, _, _, dW2 = nat.loss_grad(Wd, nfd, labd, nld, V, N, local, workspace=ws2,
                                     design=nat.DESIGN_CHUNK)
    assert torch.equal(loss, loss2) and torch.equal(dW, dW2)


SHAPES = [
    # B, T, U, V, dtype
    (3, 13, 100, 32, 'f32'),   # V = 32 path, 2 positions per lane, L = 6: chunks of 6, 6, 1
    (2, 6, 127, 32, 'f32'),    # NPG = 128, exactly one chunk
    (2, 7, 64, 32, 'bf16'),    # smallest 2-per-lane string (NPG = 66); E in its own region
    (2, 40, 63, 31, 'f32'),    # V < 32 path at C = 32; 1 position per lane at NPG = 64
    (4, 70, 5, 2, 'f32'),      # dead column lanes; long chunks: several gather passes
    (4, 25, 5, 2, 'f32'),      # ... and one partial chunk
    (2, 1, 1, 32, 'f32'),      # T = 1
]


@pytest.mark.parametrize('B,T,U,V,dt', SHAPES)
def test_chunk_marg_vs_oracle(cuda, B, T, U, V, dt):
  W, nf, lab, nl = _random_problem(B, T, U, V, seed=B * 100 + T + U + V)
  # every string reachable (a label needs a frame): the cases are finite
  nl = np.minimum(nl, nf).astype(np.int32)
  _check(cuda, W, nf, lab, nl, V, dt == 'bf16')


def test_chunk_marg_ragged(cuda):
  """Lengths that include 0 and values that are no multiple of the chunk
  length (6 at this shape); label counts that include 0 and values below U."""
  B, T, U, V = 6, 13, 100, 32
  W, _, lab, _ = _random_problem(B, T, U, V, seed=31)
  nf = np.array([13, 0, 7, 1, 12, 5], dtype=np.int32)
  nl = np.array([13, 0, 7, 1, 3, 0], dtype=np.int32)
  _check(cuda, W, nf, lab, nl, V, False)


def test_chunk_marg_peaked_rows_and_masked_arc(cuda):
  """log_softmax(10 randn) rows and one -inf arc per utterance: outside the
  strict range, so the relaxed path (the per-frame certificate) takes it."""
  orc = _orc()
  B, T, U, V = 2, 30, 20, 32
  rng = np.random.default_rng(11)
  x = 10.0 * rng.standard_normal((B, T, V + 1, V + 1))
  W = (x - np.log(np.exp(x - x.max(-1, keepdims=True)).sum(-1, keepdims=True))
       - x.max(-1, keepdims=True)).astype(np.float32)
  for b in range(B):
    W[b, rng.integers(0, T), rng.integers(0, V + 1), rng.integers(0, V + 1)] = -np.inf
  nf = np.full([B], T, np.int32)
  lab = rng.integers(1, V + 1, (B, U)).astype(np.int32)
  nl = np.full([B], U, np.int32)
  rl, _, _, rdW = orc.loss_grad(W, nf, lab, nl, V, N)
  assert np.isfinite(rl).all() and np.isfinite(rdW).all()
  _check(cuda, W, nf, lab, nl, V, False, locals_=(False,))


def test_chunk_marg_autograd_weights(cuda):
  """RecognitionLattice.backward with per-utterance weights (0 and a negative
  one among them): ck_marg_kernel with the incoming gradient set."""
  orc = _orc()
  B, T, U, V = 6, 13, 100, 32
  W, nf, lab, nl = _random_problem(B, T, U, V, seed=5)
  nl = np.minimum(nl, nf).astype(np.int32)
  assert nat.loss_grad_design(B, T, U, V, N) == nat.DESIGN_CHUNK
  table = torch.tensor(W, device=cuda, requires_grad=True)
  lat = lt.RecognitionLattice(
      context=lt.contexts.FullNGram(vocab_size=V, context_size=N),
      alignment=lt.alignments.FrameDependent(),
      weight_fn_cacher_factory=lambda _: lt.weight_fns.NullCacher(),
      weight_fn_factory=lambda _: lt.weight_fns.TableWeightFn(table))
  frames = torch.arange(T, dtype=torch.float32)[None, :, None].expand(B, T, 1).contiguous()
  loss = lat(frames.to(cuda), torch.tensor(nf), torch.tensor(lab), torch.tensor(nl))
  w = torch.tensor([0.5, 0.0, 2.0, -1.0, 3.0, 1.0], device=cuda)
  fin = torch.isfinite(loss.detach())
  (w * loss.masked_fill(~fin, 0)).sum().backward()
  rl, rlz, rnum, rdW = orc.loss_grad(W, nf, lab, nl, V, N)
  assert_loss_close(loss.detach().cpu().numpy(), rl)
  den = orc.den_grad(W, nf, V, N)[1]
  assert_grad_marginal_close(table.grad.cpu().numpy(), rdW, den, rlz, rnum,
                             weights=(w * fin).cpu().numpy())
