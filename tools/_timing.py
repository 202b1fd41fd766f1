"""The measuring procedure the *_bench.py tools share: untimed calls for
SETTLE_S seconds (default 1.0; the clock under load settles first, as bench.py
does), then event-timed batches of REPS (10) calls, BATCHES (7) of them per
timing. Importing this module imports torch; it touches the GPU only when a
function is called."""
import os
import statistics
import time

import torch

SETTLE_S = float(os.environ.get('SETTLE_S', 1.0))
BATCHES = int(os.environ.get('BATCHES', 7))
REPS = int(os.environ.get('REPS', 10))


def settle(fn):
  t0 = time.perf_counter()
  calls = 0
  while time.perf_counter() - t0 < SETTLE_S:
    fn()
    calls += 1
    if calls % 8 == 0:
      torch.cuda.synchronize()
  torch.cuda.synchronize()


def batch_ms(fn, reps=REPS):
  e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
  e0.record()
  for _ in range(reps):
    fn()
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1) / reps


def medians(fns):
  """Median ms per call of each fn and its (min, max); batches of the fns
  alternate."""
  for fn in fns:
    settle(fn)
  samples = [[] for _ in fns]
  for _ in range(BATCHES):
    for s, fn in zip(samples, fns):
      s.append(batch_ms(fn))
  return [statistics.median(s) for s in samples], [(min(s), max(s)) for s in samples]
