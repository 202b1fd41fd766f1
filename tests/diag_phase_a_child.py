"""Child process of tests/test_gpu_chunk_phase_a.py (run with LT_LIB_PATH = the
diagnostic build, which reads LT_CHUNK_GENERIC per call): every case of that
file through the specialised phase A (fp32 at V = 32) and, with
LT_CHUNK_GENERIC=1, through the run-time one, each on a 0xFF-filled
workspace, and the same for lt_chunk_forward (the strict range). loss, log_z,
num, dW and the set of utterances sent to the frame-serial kernels must be
equal bit for bit, and lt_diag_chunk_ab_spec()
must say which phase A the call launched: 1 without the switch, 0 with it,
and 0 for a bf16 and a V = 16 problem, which have no specialised form. Prints
one line per case, then 'ok'."""
import ctypes
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from last_torch_amd import _native as nat  # noqa: E402
import test_gpu_chunk_phase_a as pa  # noqa: E402


LIB = ctypes.CDLL(os.environ['LT_LIB_PATH'])  # the library _native loaded: the same handle


def _call(Wd, nfd, labd, nld, vocab, local, generic, want_spec):
  if generic:
    os.environ['LT_CHUNK_GENERIC'] = '1'
  else:
    os.environ.pop('LT_CHUNK_GENERIC', None)
  ws = pa.poisoned_ws(Wd, labd.shape[1], local)
  out = nat.loss_grad(Wd, nfd, labd, nld, vocab, pa.N, local, workspace=ws,
                      design=nat.DESIGN_CHUNK)
  torch.cuda.synchronize()
  assert LIB.lt_diag_chunk_ab_spec() == want_spec, (LIB.lt_diag_chunk_ab_spec(), want_spec)
  return out, pa.flagged_set(ws, Wd.shape[0])


def _same(name, dev, W, nf, lab, nl, vocab, bf16, locals_, want_spec, flagged=None):
  Wd = torch.tensor(W).to(torch.bfloat16 if bf16 else torch.float32).to(dev)
  nfd, labd, nld = (torch.tensor(x).to(dev) for x in (nf, lab, nl))
  for local in locals_:
    spec, fs = _call(Wd, nfd, labd, nld, vocab, local, False, want_spec)
    gen, fg = _call(Wd, nfd, labd, nld, vocab, local, True, 0)
    assert fs == fg, (name, local, fs, fg)
    if flagged is not None:
      assert fs == flagged, (name, fs, flagged)
    for what, x, y in zip(('loss', 'log_z', 'num', 'dW'), spec, gen):
      # bits, NaNs included
      assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (name, local, what)
    # lt_chunk_forward, where a chunk outside the strict range is flagged too
    os.environ.pop('LT_CHUNK_GENERIC', None)
    fspec, ss = pa.run_strict(Wd, nfd, labd, nld, local)
    assert LIB.lt_diag_chunk_ab_spec() == want_spec
    os.environ['LT_CHUNK_GENERIC'] = '1'
    fgen, sg = pa.run_strict(Wd, nfd, labd, nld, local)
    assert LIB.lt_diag_chunk_ab_spec() == 0
    assert ss == sg, (name, local, ss, sg)
    for what, x, y in zip(('loss', 'log_z', 'num'), fspec, fgen):
      assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (name, local, 'forward', what)
  print('same bits:', name, flush=True)


def main():
  dev = torch.device('cuda')
  for name, W, nf, lab, nl, locals_, flagged in pa.cases():
    _same(name, dev, W, nf, lab, nl, pa.V, False, locals_, 1, flagged)
  # no specialised form: bf16 W, and V = 16
  W, nf, lab, nl = pa._frames_case(100, 1)
  _same('bf16', dev, W, nf, lab, nl, pa.V, True, (False,), 0)
  rng = np.random.default_rng(7900)
  W16 = rng.standard_normal((3, 23, 17, 17)).astype(np.float32)
  nf16 = np.array([23, 11, 0], np.int32)
  lab16 = rng.integers(0, 17, (3, 30)).astype(np.int32)
  nl16 = np.array([20, 5, 0], np.int32)
  _same('V=16', dev, W16, nf16, lab16, nl16, 16, False, (False,), 0)
  print('ok')


if __name__ == '__main__':
  main()
