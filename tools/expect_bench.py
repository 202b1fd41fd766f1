"""Times lt_table_expectation (lt_expect.hip) against the table kernels that
`entropy` costs today. Prints one JSON line per workload and appends it to
OUT (default profiles/expect_bench.jsonl):

  den_ms        (a) lt_table_forward + lt_table_den_backward in Log: log_z,
                alpha and the arc marginals -- the yardstick
  value_ms      (b) lt_table_expectation, value only (E and log_z; the forward
                kernel, no history kept)
  grad_ms       (c) lt_table_expectation with marg and cov (both kernels)
  grad_over_den (c) / (a)

All three run on the table graph of the FullNGram context (the bigram of the
bench shape goes through its next_state_table(), as `expectation` does).
Untimed calls for SETTLE_S seconds per leg (default 1.0; the clock under load
settles first, as bench.py does), then the median over BATCHES (7)
event-timed batches of REPS (10) calls, the legs alternating batch by batch
in one process.
ONLY=fp32|bf16|trigram runs one workload.
"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from last_torch_amd import _native as nat  # noqa: E402
from last_torch_amd import contexts  # noqa: E402
from _timing import BATCHES, REPS, SETTLE_S, batch_ms, settle  # noqa: E402

OUT = os.environ.get('OUT', os.path.join(ROOT, 'profiles', 'expect_bench.jsonl'))


def run(name, V, n, B, T, dtype=torch.float32):
  context = contexts.FullNGram(vocab_size=V, context_size=n)
  table = context.next_state_table().to(torch.int32)
  C = table.shape[0]
  g = torch.Generator(device='cuda')
  g.manual_seed(0)
  W = torch.randn([B, T, C, V + 1], generator=g, device='cuda').to(dtype)
  values = torch.randn([B, T, C, V + 1], generator=g, device='cuda')
  nf = torch.full([B], T, dtype=torch.int32, device='cuda')
  graph = nat.TableGraph(table, 0, 'cuda')

  def den():
    log_z, alpha = nat.table_forward(graph, W, nf, nat.SEMIRING_LOG)
    return log_z, nat.table_den_backward(graph, W, nf, nat.SEMIRING_LOG, log_z, alpha)

  def value():
    return nat.table_expectation(graph, W, values, nf, False, False)

  def grad():
    return nat.table_expectation(graph, W, values, nf, True, True)

  log_z, marg = den()
  _, log_z2, marg2, _ = grad()
  dz = float((log_z - log_z2).abs().max())
  dm = float((marg.float() - marg2).abs().max())
  del marg, marg2
  legs = (den, value, grad)
  for leg in legs:
    settle(leg)
  ms = [[], [], []]
  for _ in range(BATCHES):
    for i, leg in enumerate(legs):
      ms[i].append(batch_ms(leg, REPS))
  a, b, c = (statistics.median(x) for x in ms)
  line = json.dumps({
      'workload': name, 'B': B, 'T': T, 'C': int(C), 'V': V, 'dtype': str(dtype).split('.')[-1],
      'den_ms': a, 'value_ms': b, 'grad_ms': c, 'grad_over_den': c / a, 'value_over_den': b / a,
      'den_min_max_ms': (min(ms[0]), max(ms[0])), 'value_min_max_ms': (min(ms[1]), max(ms[1])),
      'grad_min_max_ms': (min(ms[2]), max(ms[2])), 'log_z_max_diff': dz, 'marg_max_diff': dm,
      'batches': BATCHES, 'reps': REPS, 'settle_s': SETTLE_S,
      'device': torch.cuda.get_device_name(0)})
  print(line, flush=True)
  os.makedirs(os.path.dirname(OUT) or '.', exist_ok=True)
  with open(OUT, 'a') as f:
    f.write(line + '\n')


def main():
  if not torch.cuda.is_available():
    raise SystemExit('expect_bench.py needs a ROCm GPU')
  only = os.environ.get('ONLY')
  if only in (None, 'fp32'):
    run('FullNGram bigram V=32 through its table (bench shape)', 32, 1, 64, 1000)
  if only in (None, 'bf16'):
    run('the bench shape, bf16 W', 32, 1, 64, 1000, torch.bfloat16)
  if only in (None, 'trigram'):
    run('FullNGram trigram V=8 through its table, B=64', 8, 2, 64, 1000)


if __name__ == '__main__':
  main()
