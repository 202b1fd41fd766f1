"""Child process of tests/test_gpu_chunk_dw_exit.py (run with LT_LIB_PATH = the
diagnostic build, which reads LT_CHUNK_GENERIC per call): every fp32 V = 32
case of that file, and its fallback case, through the ck_marg_kernel
instantiation of the plan's chunk length (the straight-line exit) and through
the run-time-geometry kernel (LT_CHUNK_GENERIC=1: the exit's loop), each on
0xFF-filled outputs and workspace. loss, log_z, num, dW and the flagged set
must be bit-equal, and the library must report the kernel each call launched
(lt_diag_chunk_marg_len: the planned L, or 0). Prints one line per case, then
'ok'."""
import ctypes
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from last_torch_amd import _native as nat  # noqa: E402
from poisoned_buffers import poisoned  # noqa: E402
import test_gpu_chunk_dw_exit as dwx  # noqa: E402

LIB = ctypes.CDLL(os.environ['LT_LIB_PATH'])  # the library _native loaded: the same handle


def _call(d, V, U, local, generic, want_len):
  if generic:
    os.environ['LT_CHUNK_GENERIC'] = '1'
  else:
    os.environ.pop('LT_CHUNK_GENERIC', None)
  ws = dwx._poisoned_ws(d[0], V, U, local)
  with poisoned(nat):
    out = nat.loss_grad(*d, V, dwx.N, local, workspace=ws, design=nat.DESIGN_CHUNK)
  torch.cuda.synchronize()
  assert LIB.lt_diag_chunk_marg_len() == want_len, (LIB.lt_diag_chunk_marg_len(), want_len)
  return out + (ws[:4 * d[0].shape[0]].clone(),)


def main():
  dev = torch.device('cuda')
  todo = [(name, c, (False, True)) for name, c in dwx.spec_cases() if not c[5]]
  todo.append(('fallback', dwx._fallback_case()[:5] + (False,), (False,)))
  for name, (W, nf, lab, nl, V, bf16), locals_ in todo:
    d = dwx._dev(dev, W, nf, lab, nl, bf16)
    U = lab.shape[1]
    for local in locals_:
      spec = _call(d, V, U, local, False, dwx.SPEC_LEN[U])
      gen = _call(d, V, U, local, True, 0)
      for what, x, y in zip(('loss', 'log_z', 'num', 'dW', 'flags'), spec, gen):
        # bits, NaNs included
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (name, local, what)
    print('same bits:', name, flush=True)
  print('ok')


if __name__ == '__main__':
  main()
