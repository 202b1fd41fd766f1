"""Times the three kernels behind RecognitionLattice.sampled_risk
(lt_table_path_score, lt_table_path_scatter: lt_paths.hip; lt_edit_distance:
lt_edit.hip) against the route a user had before them. Prints one JSON line
per workload and appends it to OUT (default profiles/risk_bench.jsonl):

  score_ms           _native.table_path_score alone (weights and states) on
                     the paths lt_table_sample drew
  scatter_ms         _native.table_path_scatter alone: the dense fp32 dW
  distance_ms        _native.edit_distance alone, against references of U
                     labels
  sample_ms          _native.table_sample alone on the same problem: the call
                     these three follow, and their yardstick
  risk_fwd_bwd_ms    RecognitionLattice.sampled_risk(...)[0].sum().backward()
                     end to end: the Log forward, the sampler, the three
                     kernels and the autograd glue. The weight function hands
                     the lattice W itself (_GivenWeights), so the figure is the
                     lattice's share and not a weight function's
  torch_route_ms     cpu.path_weights (forward and backward) + cpu.edit_distance
                     on the same ROCm tensors: the definitions in torch ops,
                     Python loops over frames and over hypothesis tokens
  nonblank_share     the share of live frames on which the sampled paths emit a
                     label: the number of serial steps of the state walk and of
                     DP row updates per frame

The kernel timings: untimed calls for SETTLE_S seconds (default 1.0; the
clock under load settles first, as bench.py does), then the median over
BATCHES (7) event-timed batches of REPS (10) calls, the kernels alternating
batch by batch. The torch route takes seconds a call, so it gets one untimed
call and the median of TORCH_CALLS (3) single timed calls, run between the
kernels' batches.
ONLY=fp32|bf16|blank runs one workload.
"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import last_torch_amd as lt  # noqa: E402
from last_torch_amd import _native as nat  # noqa: E402
from last_torch_amd import cpu  # noqa: E402
from _timing import BATCHES, REPS, SETTLE_S, batch_ms, settle  # noqa: E402

TORCH_CALLS = int(os.environ.get('TORCH_CALLS', 3))
OUT = os.environ.get('OUT', os.path.join(ROOT, 'profiles', 'risk_bench.jsonl'))
SEED = 2026


class _GivenWeights(lt.weight_fns.WeightFn):
  """A weight function whose arc weights are a given [B, T, C, V+1] tensor."""
  time_batched = True

  def __init__(self, W):
    super().__init__()
    self.W = W

  def forward(self, cache, frame, state=None):
    raise NotImplementedError('_GivenWeights serves whole utterances (forward_joint)')

  def forward_joint(self, cache, frames):
    del cache, frames
    return self.W


def run(name, V, n, B, T, S, U, dtype=torch.float32, blank_bias=0.0):
  context = lt.contexts.FullNGram(vocab_size=V, context_size=n)
  table = context.next_state_table().to(torch.int32)
  C = table.shape[0]
  g = torch.Generator(device='cuda')
  g.manual_seed(0)
  W = torch.randn([B, T, C, V + 1], generator=g, device='cuda')
  W[..., 0] += blank_bias
  W = W.to(dtype)
  nf = torch.full([B], T, dtype=torch.int32, device='cuda')
  ref = torch.randint(1, V + 1, [B, U], generator=g, device='cuda', dtype=torch.int32)
  nl = torch.full([B], U, dtype=torch.int32, device='cuda')
  grad = torch.randn([B, S], generator=g, device='cuda')
  graph = nat.TableGraph(table, 0, 'cuda')
  log_z, alpha = nat.den_forward(W, nf, V, n, nat.SEMIRING_LOG)
  labels, weights = nat.table_sample(graph, W, nf, log_z, alpha, S, SEED)
  _, states = nat.table_path_score(graph, W, nf, labels)

  Wg = W.clone().requires_grad_(True)
  lattice = lt.RecognitionLattice(
      context=context, alignment=lt.alignments.FrameDependent(),
      weight_fn_cacher_factory=lambda _: lt.weight_fns.NullCacher(),
      weight_fn_factory=lambda _: _GivenWeights(Wg))
  frames = torch.zeros([B, T, 1], device='cuda')

  def sample():
    return nat.table_sample(graph, W, nf, log_z, alpha, S, SEED)

  def score():
    return nat.table_path_score(graph, W, nf, labels)

  def scatter():
    return nat.table_path_scatter(graph, W, nf, labels, states, grad)

  def distance():
    return nat.edit_distance(labels, nf, ref, nl)

  def risk():
    Wg.grad = None
    lattice.sampled_risk(frames, nf, ref, nl, S, SEED)[0].sum().backward()

  def torch_route():
    Wt = W.detach().float().requires_grad_(True)  # bf16 widened exactly
    pw, _ = cpu.path_weights(Wt, nf, labels, context)
    pw.backward(grad)
    return pw, Wt.grad, cpu.edit_distance(labels, nf, ref, nl)[0]

  # the two routes agree before anything is timed
  pw, dW_t, dist_t = torch_route()  # also the torch route's untimed call
  assert torch.equal(score()[0], weights) and torch.equal(pw.detach(), weights)
  assert torch.equal(distance()[0], dist_t)
  assert torch.allclose(scatter(), dW_t, rtol=0,
                        atol=S * 2.0**-24 * float(grad.abs().sum(1).max()))
  kernels = {'score': score, 'scatter': scatter, 'distance': distance, 'sample': sample,
             'risk_fwd_bwd': risk}
  for fn in kernels.values():
    settle(fn)
  ms = {k: [] for k in kernels}
  t_ms = []
  for i in range(BATCHES):
    for k, fn in kernels.items():
      ms[k].append(batch_ms(fn, REPS))
    if i < TORCH_CALLS:
      t_ms.append(batch_ms(torch_route, 1))
  med = {k: statistics.median(v) for k, v in ms.items()}
  three = med['score'] + med['scatter'] + med['distance']
  line = {'workload': name, 'B': B, 'T': T, 'S': S, 'U': U, 'C': int(C), 'V': V,
          'dtype': str(dtype).split('.')[-1], 'blank_bias': blank_bias,
          'nonblank_share': float((labels > 0).float().mean())}
  line.update({f'{k}_ms': v for k, v in med.items()})
  line.update({'three_kernels_ms': three, 'three_over_sample': three / med['sample'],
               'torch_route_ms': statistics.median(t_ms),
               'three_over_torch_route': three / statistics.median(t_ms)})
  line.update({f'{k}_min_max_ms': (min(v), max(v)) for k, v in ms.items()})
  line.update({'torch_route_min_max_ms': (min(t_ms), max(t_ms)), 'batches': BATCHES,
               'reps': REPS, 'torch_calls': len(t_ms), 'settle_s': SETTLE_S,
               'device': torch.cuda.get_device_name(0)})
  text = json.dumps(line)
  print(text, flush=True)
  os.makedirs(os.path.dirname(OUT), exist_ok=True)
  with open(OUT, 'a') as f:
    f.write(text + '\n')


def main():
  if not torch.cuda.is_available():
    raise SystemExit('risk_bench.py needs a ROCm GPU')
  only = os.environ.get('ONLY')
  if only in (None, 'fp32'):
    run('FullNGram bigram V=32 (bench shape), S=16, U=100', 32, 1, 64, 1000, 16, 100)
  if only in (None, 'bf16'):
    run('the bench shape, bf16 W', 32, 1, 64, 1000, 16, 100, torch.bfloat16)
  if only in (None, 'blank'):
    run('the bench shape, blank weights + 6 (few labels a path)', 32, 1, 64, 1000, 16, 100,
        blank_bias=6.0)


if __name__ == '__main__':
  main()
