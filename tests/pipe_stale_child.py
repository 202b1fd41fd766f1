"""Child process of tests/test_gpu_buffer_hygiene.py: stale granule tags in
the fused pipe's workspace (lt_pipe.hip, mid mode), on the normal library.

A granule is {value, tag} with tag = epoch * T + t, and the epoch counts the
process's fused calls from zero. Call 1 (epoch 1) runs problem A with 2T
frames: its tags are 2T + t'. Call 2 (epoch 2) runs problem B with T frames in
the same workspace: the tags it waits for are 2T + t. For utterance 0 every
granule address of B therefore already holds the awaited tag, next to a value
of A's. Only the zeroed band and the order in which pipe_kernel's marginal
workgroups reach the frames keep B from consuming them. Checks that the
workspace is in that state, then B's loss and every dW element against the
oracle, and the hand-off error word. Prints 'ok'."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from golden_cases import assert_grad_marginal_close, assert_loss_close  # noqa: E402
from last_torch_amd import _native as nat  # noqa: E402
from oracle import oracle as orc  # noqa: E402  (test infrastructure only)


def main():
  B, T, U, V, n = 4, 48, 10, 32, 1
  C = V + 1
  dev = torch.device('cuda')
  rng = np.random.default_rng(48)
  d = nat.DESIGN_FUSED_PIPE

  def problem(frames, nf, nl):
    W = rng.standard_normal((B, frames, C, C)).astype(np.float32)
    lab = rng.integers(0, V + 1, (B, U)).astype(np.int32)
    return W, np.array(nf, np.int32), lab, np.array(nl, np.int32)

  pa = problem(2 * T, [2 * T] * B, [U] * B)
  pb = problem(T, [T, T - 1, 1, 0], [U, 3, 1, 0])
  da, db = (tuple(torch.tensor(x, device=dev) for x in p) for p in (pa, pb))
  nbytes = max(nat.loss_grad_workspace_bytes(p[0], V, n, U, False, d) for p in (da, db))
  ws = torch.zeros([nbytes], dtype=torch.uint8, device=dev)

  nat.loss_grad(*da, V, n, False, workspace=ws, design=d)  # epoch 1
  torch.cuda.synchronize()
  assert nat.grad_workspace_errors(ws, da[0], V, n, U, False) == 0
  # the alpha granules of utterance 0, as B will address them: [T, C] from the
  # workspace's start, tag in the high word
  tags = (ws[:8 * T * C].view(torch.int64).reshape(T, C) >> 32).cpu().numpy()
  want = 2 * T + np.arange(T)[:, None]
  stale_rows = int((tags == want).any(axis=1).sum())
  assert stale_rows > 0, 'problem A left no granule with a tag problem B waits for'

  loss, lz, num, dW = nat.loss_grad(*db, V, n, False, workspace=ws, design=d)  # epoch 2
  torch.cuda.synchronize()
  assert nat.grad_workspace_errors(ws, db[0], V, n, U, False) == 0
  W, nf, lab, nl = pb
  rl, rlz, rnum, rdW = orc.loss_grad(W, nf, lab, nl, V, n)
  den = orc.den_grad(W, nf, V, n)[1]
  assert_loss_close(loss.cpu().numpy(), rl)
  assert_loss_close(lz.cpu().numpy(), rlz)
  assert_loss_close(num.cpu().numpy(), rnum)
  assert_grad_marginal_close(dW.cpu().numpy(), rdW, den, rlz, rnum)
  print(f'ok: {stale_rows} of {T} alpha rows of utterance 0 held the awaited tags')


if __name__ == '__main__':
  main()
