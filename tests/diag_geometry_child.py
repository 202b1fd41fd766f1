"""Child process of tests/test_gpu_chunk_geometry.py (run with LT_LIB_PATH =
the diagnostic build, which reads LT_CHUNK_GENERIC per call): for every shape
of that file, one chunked lt_loss_grad call through the ck_marg_kernel
instantiation of the plan's chunk length (fp32 at V = 32; bf16 and V < 32
have none) and one with LT_CHUNK_GENERIC=1 (the run-time-geometry kernel),
each on a NaN-poisoned workspace. loss, log_z, num and dW must be bit-equal,
and the library must report the kernel each call launched
(lt_diag_chunk_marg_len: the planned L, or 0). Prints one line per case,
then 'ok'."""
import ctypes
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from last_torch_amd import _native as nat  # noqa: E402
import test_gpu_chunk_geometry as geo  # noqa: E402


LIB = ctypes.CDLL(os.environ['LT_LIB_PATH'])  # the library _native loaded: the same handle


def _call(Wd, nfd, labd, nld, V, U, local, generic, want_len):
  if generic:
    os.environ['LT_CHUNK_GENERIC'] = '1'
  else:
    os.environ.pop('LT_CHUNK_GENERIC', None)
  ws = geo._poisoned_ws(Wd, V, U, local)
  out = nat.loss_grad(Wd, nfd, labd, nld, V, geo.N, local, workspace=ws, design=nat.DESIGN_CHUNK)
  torch.cuda.synchronize()
  assert nat.chunk_fallback_count(ws, Wd.shape[0]) == 0
  # the kernel phase C launched: the instantiation of that chunk length, or 0
  assert LIB.lt_diag_chunk_marg_len() == want_len, (LIB.lt_diag_chunk_marg_len(), want_len)
  return out


def main():
  dev = torch.device('cuda')
  for name, (W, nf, lab, nl, V, bf16) in geo.cases():
    Wd = torch.tensor(W).to(torch.bfloat16 if bf16 else torch.float32).to(dev)
    nfd, labd, nld = (torch.tensor(x).to(dev) for x in (nf, lab, nl))
    U = lab.shape[1]
    # fp32 at V = 32 takes the instantiation of the plan's L; bf16 and V < 32 have none
    want = geo.CHUNK_LEN[U] if (V == 32 and not bf16) else 0
    for local in (False, True):
      spec = _call(Wd, nfd, labd, nld, V, U, local, False, want)
      gen = _call(Wd, nfd, labd, nld, V, U, local, True, 0)
      for what, x, y in zip(('loss', 'log_z', 'num', 'dW'), spec, gen):
        # bits, NaNs included (an unreachable string's loss is +inf, never NaN)
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (name, local, what)
    print('same bits:', name, flush=True)
  print('ok')


if __name__ == '__main__':
  main()
