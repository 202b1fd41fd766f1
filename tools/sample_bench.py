"""Times path sampling (lt_table_sample, lt_sample.hip) against the route a
user had before it. Prints one JSON line per workload:

  sample_ms          _native.table_sample alone: one launch, S walks per
                     utterance over a given alpha
  forward_ms         the alpha pass it needs (lt_den_forward in Log, for
                     FullNGram x FrameDependent)
  torch_route_ms     cpu.sample on the same ROCm tensors and the same alpha:
                     the definition in torch ops, a Python loop over frames
  paths_equal_share  the share of (utterance, sample) paths on which the two
                     routes agree frame for frame; their logf differ in the
                     last bits, so near-ties may differ: reported, not
                     asserted

The kernel timings: untimed calls for SETTLE_S seconds (default 1.0; the
clock under load settles first, as bench.py does), then the median over
BATCHES (7) event-timed batches of REPS (10) calls, the two kernels
alternating batch by batch. The torch route takes seconds a call, so it gets
one untimed call and the median of TORCH_CALLS (3) single timed calls, run
between the kernels' batches.
ONLY=s1|s16|s64|bf16|trigram runs one workload.
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
from last_torch_amd import cpu  # noqa: E402
from _timing import BATCHES, REPS, SETTLE_S, batch_ms, settle  # noqa: E402

TORCH_CALLS = int(os.environ.get('TORCH_CALLS', 3))
SEED = 2026


def run(name, V, n, B, T, S, dtype=torch.float32):
  context = contexts.FullNGram(vocab_size=V, context_size=n)
  table = context.next_state_table().to(torch.int32)
  C = table.shape[0]
  g = torch.Generator(device='cuda')
  g.manual_seed(0)
  W = torch.randn([B, T, C, V + 1], generator=g, device='cuda').to(dtype)
  nf = torch.full([B], T, dtype=torch.int32, device='cuda')
  graph = nat.TableGraph(table, 0, 'cuda')

  def forward():
    return nat.den_forward(W, nf, V, n, nat.SEMIRING_LOG)

  log_z, alpha = forward()

  def sample():
    return nat.table_sample(graph, W, nf, log_z, alpha, S, SEED)

  def torch_route():
    return cpu.sample(W, nf, context, S, SEED, log_z=log_z, alpha=alpha)

  labels, _ = sample()
  ref_labels, _, _ = torch_route()  # also the torch route's untimed call
  share = float((labels == ref_labels).all(dim=-1).float().mean())
  settle(sample)
  settle(forward)
  s_ms, f_ms, t_ms = [], [], []
  for i in range(BATCHES):
    s_ms.append(batch_ms(sample, REPS))
    f_ms.append(batch_ms(forward, REPS))
    if i < TORCH_CALLS:
      t_ms.append(batch_ms(torch_route, 1))
  s_med, f_med, t_med = (statistics.median(x) for x in (s_ms, f_ms, t_ms))
  print(json.dumps({
      'workload': name, 'B': B, 'T': T, 'S': S, 'C': int(C), 'V': V,
      'dtype': str(dtype).split('.')[-1], 'sample_ms': s_med, 'forward_ms': f_med,
      'torch_route_ms': t_med, 'sample_over_torch_route': s_med / t_med,
      'paths_equal_share': share, 'sample_min_max_ms': (min(s_ms), max(s_ms)),
      'torch_route_min_max_ms': (min(t_ms), max(t_ms)), 'batches': BATCHES, 'reps': REPS,
      'torch_calls': len(t_ms), 'settle_s': SETTLE_S,
      'device': torch.cuda.get_device_name(0)}), flush=True)


def main():
  if not torch.cuda.is_available():
    raise SystemExit('sample_bench.py needs a ROCm GPU')
  only = os.environ.get('ONLY')
  for key, S in (('s1', 1), ('s16', 16), ('s64', 64)):
    if only in (None, key):
      run(f'FullNGram bigram V=32 (bench shape), S={S}', 32, 1, 64, 1000, S)
  if only in (None, 'bf16'):
    run('the bench shape, bf16 W, S=16', 32, 1, 64, 1000, 16, torch.bfloat16)
  if only in (None, 'trigram'):
    run('FullNGram trigram V=32, B=8, S=16', 32, 2, 8, 1000, 16)


if __name__ == '__main__':
  main()
