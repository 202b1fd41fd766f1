"""Times forced alignment (lt_table_align, lt_align.hip) against the dense
route it replaces. Prints one JSON line per workload:

  align_ms            _native.table_align: one launch, forward + backtrace
  dense_route_ms      RecognitionLattice._align_dense on the same inputs:
                      lt_table_num_backward in MaxTropical (memset + dense
                      one-hot dW [B,T,C,V+1]) and the torch compaction -- the
                      way to the same answer before lt_table_align
  num_forward_max_ms  the MaxTropical string distance alone (lt_num_forward
                      for FullNGram x FrameDependent, else
                      lt_table_num_forward): the chain without a path; for
                      information
  outputs_equal       the two routes agree on all three outputs

Each timing: untimed calls for SETTLE_S seconds (default 1.0; the clock under
load settles first, as bench.py does), then the median over BATCHES (7)
event-timed batches of REPS (10) calls. The routes alternate batch by batch.
ONLY=bench|bf16|t2000|fld2 runs one workload.
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from last_torch_amd import _native as nat  # noqa: E402
from last_torch_amd import contexts  # noqa: E402
from last_torch_amd.lattices import RecognitionLattice  # noqa: E402
from _timing import BATCHES, REPS, SETTLE_S, batch_ms, medians  # noqa: E402



def run(name, V, n, K, B, T, U, dtype=torch.float32):
  table = contexts.FullNGram(vocab_size=V, context_size=n).next_state_table().to(torch.int32)
  C = table.shape[0]
  g = torch.Generator(device='cuda')
  g.manual_seed(0)
  W = torch.randn([B, T, C, V + 1], generator=g, device='cuda').to(dtype)
  nf = torch.full([B], T, dtype=torch.int32, device='cuda')
  lab = torch.randint(1, V + 1, (B, U), generator=g, device='cuda', dtype=torch.int32)
  nl = torch.full([B], U, dtype=torch.int32, device='cuda')
  graph = nat.TableGraph(table, K, 'cuda')

  def align():
    return nat.table_align(graph, W, nf, lab, nl)

  def dense():
    return RecognitionLattice._align_dense(graph, W, nf, lab, nl)

  def forward():
    if K == 0:
      return nat.num_forward(W, nf, lab, nl, V, n, nat.SEMIRING_MAX, want_alpha=False)
    return nat.table_num_forward(graph, W, nf, lab, nl, nat.SEMIRING_MAX)

  equal = all(bool(torch.equal(x, y)) for x, y in zip(align(), dense()))
  (a_ms, d_ms, f_ms), spread = medians([align, dense, forward])
  print(json.dumps({
      'workload': name, 'B': B, 'T': T, 'U': U, 'C': int(C), 'V': V, 'K': K,
      'dtype': str(dtype).split('.')[-1], 'align_ms': a_ms, 'dense_route_ms': d_ms,
      'num_forward_max_ms': f_ms, 'align_over_dense': a_ms / d_ms,
      'align_min_max_ms': spread[0], 'dense_min_max_ms': spread[1], 'outputs_equal': equal,
      'batches': BATCHES, 'reps': REPS, 'settle_s': SETTLE_S,
      'device': torch.cuda.get_device_name(0)}), flush=True)


def main():
  if not torch.cuda.is_available():
    raise SystemExit('align_bench.py needs a ROCm GPU')
  only = os.environ.get('ONLY')
  if only in (None, 'bench'):
    run('FrameDependent x FullNGram bigram V=32 (bench shape)', 32, 1, 0, 64, 1000, 100)
  if only in (None, 'bf16'):
    run('the bench shape, bf16 W', 32, 1, 0, 64, 1000, 100, torch.bfloat16)
  if only in (None, 't2000'):
    run('FrameDependent x FullNGram bigram V=32, T=2000, U=127', 32, 1, 0, 64, 2000, 127)
  if only in (None, 'fld2'):
    run('FrameLabelDependent(2) x FullNGram bigram V=32 (bench shape)', 32, 1, 2, 64, 1000, 100)


if __name__ == '__main__':
  main()
