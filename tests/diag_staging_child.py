"""Child process of tests/test_gpu_chunk_staging.py (run with LT_LIB_PATH =
the diagnostic build and LT_CHUNK_FUSE=0, which that build reads per call):
the unfused route at a small batch -- phase A alone in its launch,
ck_combine_kernel after it, phase C polling walks that finish in its own
launch -- on the ragged shapes of that file, against the C oracle. Prints one
line per case, then 'ok'."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from last_torch_amd import _native as nat  # noqa: E402
import test_gpu_chunk_staging as stg  # noqa: E402


def main():
  assert os.environ.get('LT_CHUNK_FUSE') == '0'
  dev = torch.device('cuda')
  for U, V, bf16 in ((63, 32, False), (1, 32, True), (63, 16, False)):
    W, nf, lab, nl = stg._ragged(U, V, bf16, seed=4900 + U + V)
    W, nf, lab, nl = W[:3], nf[[5, 2, 1]].copy(), lab[:3], nl[[5, 2, 1]].copy()
    W = stg._host(W, bf16)
    Wd, nfd, labd, nld = stg._dev(dev, W, nf, lab, nl, bf16)
    for local in (False, True):
      out, ws = stg._loss_grad(Wd, nfd, labd, nld, V, local)
      stg._assert_close(out, stg._ref(('child', U, V, bf16), W, nf, lab, nl, V, local), bf16)
      assert nat.chunk_fallback_count(ws, 3) == 0
    print('unfused:', U, V, 'bf16' if bf16 else 'f32', flush=True)
  print('ok')


if __name__ == '__main__':
  main()
