"""Times prefix beam search (lt_table_beam_search, lt_beam.hip) against the
route a user had before it and against the one decoder there was. Prints one
JSON line per workload (profiles/beam_bench.jsonl keeps a run:
`python tools/beam_bench.py > profiles/beam_bench.jsonl`):

  beam_ms            _native.table_beam_search alone: one launch, one wave per
                     utterance, the label sequences read back in the launch
  torch_route_ms     cpu.beam_search on the same ROCm tensors: the definition
                     in torch ops, a Python loop over frames
  shortest_path_ms   _native.viterbi on the same weights: the best alignment
                     path, the decoder the package had
  beams_equal_share  the share of utterances whose whole beam (labels, lengths)
                     agrees between the two routes. MaxTropical scores are
                     fp32 adds and maxes, so it must be 1 and the scores equal
                     bit for bit (asserted); in Log the two logaddexp differ
                     in the last bits and near-ties may differ: reported

The shape is bench.py's: B = 64, T = 1000, FullNGram bigram V = 32, N(0, 1)
weights with a blank bias of 3 (with it beams hold prefixes together with
their parents, so the merge works). K in {4, 16, 64} x {Log, MaxTropical} x
{fp32, bf16}.

The kernel timings: untimed calls for SETTLE_S seconds (default 1.0; the
clock under load settles first, as bench.py does), then the median over
BATCHES (7) event-timed batches of REPS (10) calls, the two kernels
alternating batch by batch. The torch route takes seconds a call, so it gets
one untimed call and the median of TORCH_CALLS (2) single timed calls, run
between the kernels' batches.
ONLY=k4|k16|k64 runs one beam size.
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
from last_torch_amd import semirings  # noqa: E402
from _timing import BATCHES, REPS, SETTLE_S, batch_ms, settle  # noqa: E402

TORCH_CALLS = int(os.environ.get('TORCH_CALLS', 2))
BLANK_BIAS = 3.0


def run(V, n, B, T, K, semiring, dtype):
  context = contexts.FullNGram(vocab_size=V, context_size=n)
  table = context.next_state_table().to(torch.int32)
  C = table.shape[0]
  g = torch.Generator(device='cuda')
  g.manual_seed(0)
  W = torch.randn([B, T, C, V + 1], generator=g, device='cuda')
  W[..., 0] += BLANK_BIAS
  W = W.to(dtype)
  nf = torch.full([B], T, dtype=torch.int32, device='cuda')
  graph = nat.TableGraph(table, 0, 'cuda')
  sid = nat.SEMIRING_LOG if semiring is semirings.Log else nat.SEMIRING_MAX
  if not nat.table_beam_search_supported(graph, W, K):
    raise SystemExit(f'lt_table_beam_search does not take K={K}')

  def beam():
    return nat.table_beam_search(graph, W, nf, K, sid)

  def torch_route():
    return cpu.beam_search(W, nf, context, K, semiring)

  def shortest_path():
    return nat.viterbi(W, nf, V, n, nat.LABELS_TRUE)

  labels, nl, scores = beam()
  rl, rn, rs = torch_route()  # also the torch route's untimed call
  same = (labels == rl).all(dim=-1).all(dim=-1) & (nl.long() == rn).all(dim=-1)
  share = float(same.float().mean())
  if semiring is semirings.MaxTropical:
    assert share == 1.0 and torch.equal(scores, rs), 'MaxTropical beams must be bit-equal'
  gap = (scores - rs)[torch.isfinite(rs) & same[:, None]].abs()
  worst = float(gap.max()) if gap.numel() else 0.0
  settle(beam)
  settle(shortest_path)
  b_ms, v_ms, t_ms = [], [], []
  for i in range(BATCHES):
    b_ms.append(batch_ms(beam, REPS))
    v_ms.append(batch_ms(shortest_path, REPS))
    if i < TORCH_CALLS:
      t_ms.append(batch_ms(torch_route, 1))
  b_med, v_med, t_med = (statistics.median(x) for x in (b_ms, v_ms, t_ms))
  print(json.dumps({
      'workload': f'FullNGram bigram V={V} (bench shape), K={K}, {semiring.name}', 'B': B, 'T': T,
      'K': K, 'C': int(C), 'V': V, 'semiring': semiring.name,
      'dtype': str(dtype).split('.')[-1], 'beam_ms': b_med, 'torch_route_ms': t_med,
      'shortest_path_ms': v_med, 'beam_over_torch_route': b_med / t_med,
      'beam_over_shortest_path': b_med / v_med, 'beams_equal_share': share,
      'worst_score_gap_on_equal_beams': worst, 'beam_min_max_ms': (min(b_ms), max(b_ms)),
      'torch_route_min_max_ms': (min(t_ms), max(t_ms)), 'batches': BATCHES, 'reps': REPS,
      'torch_calls': len(t_ms), 'settle_s': SETTLE_S, 'blank_bias': BLANK_BIAS,
      'device': torch.cuda.get_device_name(0)}), flush=True)


def main():
  if not torch.cuda.is_available():
    raise SystemExit('beam_bench.py needs a ROCm GPU')
  only = os.environ.get('ONLY')
  for K in (4, 16, 64):
    if only not in (None, f'k{K}'):
      continue
    for semiring in (semirings.Log, semirings.MaxTropical):
      for dtype in (torch.float32, torch.bfloat16):
        run(32, 1, 64, 1000, K, semiring, dtype)


if __name__ == '__main__':
  main()
