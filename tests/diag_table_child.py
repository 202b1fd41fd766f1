"""Child of tests/test_gpu_table_paths.py::test_diag_switches: the general
table kernels under one of the diagnostic build's switches (LT_LIB_PATH = the
diagnostic build) -- LT_TAB_BT_SERIAL=1, the one-thread-per-utterance Viterbi
backtrace (tab_backtrace_kernel), or LT_TAB_THREADS=512, 512 threads on C = 7
and C = 40 states. Random tables, K = 0 and 2, utterances of T, 1 and 0
frames: Viterbi labels and weights bit-exact against the table oracle under
both label conventions, loss and dW under the per-element marginal bound.
Prints 'ok' on success."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from golden_cases import (assert_grad_marginal_close, assert_loss_close,  # noqa: E402
                          table_den_marginals)
from last_torch_amd import _native as nat  # noqa: E402
from oracle import oracle as orc  # noqa: E402  (test infrastructure only)


def main():
  serial = os.environ.get('LT_TAB_BT_SERIAL') == '1'
  wide = os.environ.get('LT_TAB_THREADS') == '512'
  assert serial != wide, 'run with exactly one of LT_TAB_BT_SERIAL=1, LT_TAB_THREADS=512'
  assert 'liblt_lattice_diag' in os.environ.get('LT_LIB_PATH', ''), 'needs the diagnostic build'
  dev = torch.device('cuda', 0)
  B, T, U, V = 3, 14, 5, 4
  for C in (7, 40):
    for K in (0, 2):
      rng = np.random.default_rng(1000 * C + K)
      table = rng.integers(0, C, (C, V)).astype(np.int32)
      W = rng.standard_normal((B, T, C, V + 1)).astype(np.float32)
      nf = np.array([T, 1, 0], np.int32)
      lab = rng.integers(0, V + 1, (B, U)).astype(np.int32)
      nl = np.array([U, 1, 0], np.int32)
      g = nat.TableGraph(table, K, dev)
      Wd = torch.tensor(W).to(dev)
      nfd, labd, nld = (torch.tensor(x).to(dev) for x in (nf, lab, nl))
      for conv in (0, 1):
        labels, w = nat.table_viterbi(g, Wd, nfd, conv)
        rlab, rw = orc.tab_viterbi(table, W, nf, K, conv)
        np.testing.assert_array_equal(w.cpu().numpy(), rw)
        np.testing.assert_array_equal(labels.cpu().numpy(), rlab)
      if wide:
        loss, lz, num, dW = nat.table_loss_grad(g, Wd, nfd, labd, nld, False)
        rl, rlz, rnum, rdW = orc.tab_loss_grad(table, W, nf, lab, nl, K)
        assert_loss_close(loss.cpu().numpy(), rl)
        assert_loss_close(lz.cpu().numpy(), rlz)
        assert_grad_marginal_close(dW.cpu().numpy(), rdW,
                                   table_den_marginals(orc, table, W, nf, lab, nl, K), rlz, rnum)
  print('ok:', 'serial backtrace' if serial else '512 threads')


if __name__ == '__main__':
  main()
