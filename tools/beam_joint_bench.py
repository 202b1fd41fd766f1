"""Times the fused joint beam search (lt_joint_beam_search, lt_beam_joint.hip)
against the pair it replaces, lt_joint_weights_ex + lt_table_beam_search, on
the same inputs. Prints one JSON line per workload
(profiles/beam_joint_bench.jsonl keeps a run:
`python tools/beam_joint_bench.py > profiles/beam_joint_bench.jsonl`):

  fused_ms         _native.joint_beam_search: the pre-pass and the search, W
                   never in memory
  pair_ms          _native.joint_weights (fp32 W, split products) followed by
                   _native.table_beam_search on it
  weights_ms       the producer's part of pair_ms, timed alone
  w_bytes          the W the pair writes and reads back
  outputs_equal    labels, lengths and scores of the two routes bit-equal
                   (asserted: the projections are N(0, 1), far inside +-40)

The shape is bench.py's: B = 64, T = 1000, V = 32, N(0, 1) projections, a
blank bias of 3 (as tools/beam_bench.py), Log, H in {128, 512}, K in {4, 16,
64}, FullNGram bigram (C = 33) and trigram (C = 1,057). The 4-gram
(C = 33,825) runs fused at B = 64, where W would be 286 GB; its pair runs at
B = 1 (4.5 GB of W), all that fits, next to the fused search at B = 1 on the
same utterance. A last line runs RecognitionLattice.beam_search on the 4-gram
at B = 64 with default settings (lattice_fusion = 'auto').

Timing as tools/_timing.py: untimed calls for SETTLE_S seconds, then the
median over BATCHES event-timed batches of REPS calls, the routes alternating
batch by batch. ONLY=bigram|trigram|fourgram|api runs one part.
"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import last_torch_amd as lt  # noqa: E402
from last_torch_amd import _native as nat  # noqa: E402
from _timing import BATCHES, REPS, SETTLE_S, medians  # noqa: E402

BLANK_BIAS = 3.0
V, T = 32, 1000
NAMES = {1: 'bigram', 2: 'trigram', 3: 'fourgram'}


def inputs(C, H, B):
  g = torch.Generator(device='cuda')
  g.manual_seed(0)
  pc = torch.randn([C, H], generator=g, device='cuda')
  pf = torch.randn([B, T, H], generator=g, device='cuda')
  wo = torch.randn([V + 1, H], generator=g, device='cuda') / H ** 0.5
  bias = torch.randn([V + 1], generator=g, device='cuda')
  bias[0] += BLANK_BIAS
  return pc, pf, wo, bias


def run(n, graph, H, K, B, pair_B):
  """Fused at batch B; the pair (and a fused run beside it) at pair_B."""
  C = graph.C
  pc, pf, wo, bias = inputs(C, H, B)
  nf = torch.full([B], T, dtype=torch.int32, device='cuda')
  pfp, nfp = pf[:pair_B].contiguous(), nf[:pair_B]
  sid = nat.SEMIRING_LOG
  if not nat.joint_beam_search_supported(graph, B, T, H, K):
    raise SystemExit(f'lt_joint_beam_search does not take H={H}, K={K}')

  def fused():
    return nat.joint_beam_search(graph, pc, pf, wo, bias, nf, K, sid)

  def fused_small():
    return nat.joint_beam_search(graph, pc, pfp, wo, bias, nfp, K, sid)

  def weights():
    return nat.joint_weights(pc, pfp, wo, bias)

  def pair():
    return nat.table_beam_search(graph, weights(), nfp, K, sid)

  equal = all(torch.equal(a, b) for a, b in zip(fused_small(), pair()))
  assert equal, 'the fused search must return the materialised pair\'s beams bit for bit'
  fns = [fused, pair, weights] + ([fused_small] if pair_B != B else [])
  med, spread = medians(fns)
  rec = {
      'workload': f'FullNGram {NAMES[n]} V={V}, H={H}, K={K}, Log', 'B': B, 'T': T, 'K': K,
      'C': C, 'V': V, 'H': H, 'precision': 'fp32', 'fused_ms': med[0], 'pair_B': pair_B,
      'pair_ms': med[1], 'weights_ms': med[2], 'w_bytes': 4 * pair_B * T * C * (V + 1),
      'fused_min_max_ms': spread[0], 'pair_min_max_ms': spread[1], 'outputs_equal': equal,
      'batches': BATCHES, 'reps': REPS, 'settle_s': SETTLE_S, 'blank_bias': BLANK_BIAS,
      'device': torch.cuda.get_device_name(0)}
  if pair_B != B:
    rec['fused_at_pair_B_ms'] = med[3]
    rec['fused_over_pair_at_pair_B'] = med[3] / med[1]
  else:
    rec['fused_over_pair'] = med[0] / med[1]
  print(json.dumps(rec), flush=True)


def api_fourgram(B=64, H=512, K=8):
  """RecognitionLattice.beam_search, default settings, where W cannot exist."""
  context = lt.contexts.FullNGram(vocab_size=V, context_size=3)
  torch.manual_seed(0)
  lat = lt.RecognitionLattice(
      context=context, alignment=lt.alignments.FrameDependent(),
      weight_fn_cacher_factory=lambda c: lt.weight_fns.SharedEmbCacher(c.num_states(), 128,
                                                                       device='cuda'),
      weight_fn_factory=lambda c: lt.weight_fns.JointWeightFn(V, H, device='cuda'))
  frames = torch.randn([B, T, 80], device='cuda')
  nf = torch.full([B], T, device='cuda')
  free, _ = torch.cuda.mem_get_info()
  lat.beam_search(frames, nf, K)   # lazy layers, the graph's device copy
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  labels, nl, scores = lat.beam_search(frames, nf, K)
  torch.cuda.synchronize()
  ms = 1e3 * (time.perf_counter() - t0)
  assert bool(torch.isfinite(scores).all()) and tuple(labels.shape) == (B, K, T)
  print(json.dumps({
      'workload': f"RecognitionLattice.beam_search, FullNGram fourgram V={V}, H={H}, K={K}, "
                  "lattice_fusion='auto'", 'B': B, 'T': T, 'K': K, 'C': context.num_states(),
      'H': H, 'call_ms_host_clock': ms, 'w_bytes': 4 * B * T * context.num_states() * (V + 1),
      'free_bytes_before': free, 'mean_labels_of_best': float(nl[:, 0].float().mean()),
      'device': torch.cuda.get_device_name(0)}), flush=True)


def main():
  if not torch.cuda.is_available():
    raise SystemExit('beam_joint_bench.py needs a ROCm GPU')
  only = os.environ.get('ONLY')
  for n in (1, 2, 3):
    if only not in (None, NAMES[n]):
      continue
    table = lt.contexts.FullNGram(vocab_size=V, context_size=n).next_state_table()
    graph = nat.TableGraph(table.to(torch.int32), 0, 'cuda')
    for H in (128, 512):
      for K in (4, 16, 64):
        run(n, graph, H, K, 64, 1 if n == 3 else 64)
  if only in (None, 'api'):
    api_fourgram()


if __name__ == '__main__':
  main()
