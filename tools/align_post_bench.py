"""Times the emission posteriors (lt_table_align_posteriors, lt_align_post.hip)
against its neighbours on the same inputs. Prints one JSON line per workload:

  align_post_ms        _native.table_align_posteriors: one launch, alpha and
                       beta waves meeting at the midpoint, emission [B,T,U]
  align_ms             _native.table_align: its MaxTropical sibling (forced
                       alignment, forward + backtrace in one launch)
  loss_grad_local_ms   _native.table_loss_grad with local normalisation: the
                       dense Log string marginals [B,T,C,V+1] -- more bytes,
                       and positions that share (state, label) stay merged
  restatement_ms       cpu.align_posteriors on the device (autograd through
                       the frame loop in torch ops): what
                       RecognitionLattice.align_posteriors runs past the
                       kernel's range
  max_abs_diff         kernel emission against the restatement's

Each kernel timing: untimed calls for SETTLE_S seconds (default 1.0; the clock
under load settles first, as bench.py does), then the median over BATCHES (7)
event-timed batches of REPS (10) calls; the three kernels alternate batch by
batch. The restatement takes a fraction of a second per call: one warm-up,
then the median of RESTATE_CALLS (3) single calls.
ONLY=bench|bf16 runs one workload.
"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from last_torch_amd import _native as nat  # noqa: E402
from last_torch_amd import alignments  # noqa: E402
from last_torch_amd import contexts  # noqa: E402
from last_torch_amd import cpu  # noqa: E402
from _timing import BATCHES, REPS, SETTLE_S, batch_ms, medians  # noqa: E402

RESTATE_CALLS = int(os.environ.get('RESTATE_CALLS', 3))


def run(name, V, n, B, T, U, dtype=torch.float32):
  table = contexts.FullNGram(vocab_size=V, context_size=n).next_state_table().to(torch.int32)
  C = table.shape[0]
  g = torch.Generator(device='cuda')
  g.manual_seed(0)
  W = torch.randn([B, T, C, V + 1], generator=g, device='cuda').to(dtype)
  nf = torch.full([B], T, dtype=torch.int32, device='cuda')
  lab = torch.randint(1, V + 1, (B, U), generator=g, device='cuda', dtype=torch.int32)
  nl = torch.full([B], U, dtype=torch.int32, device='cuda')
  graph = nat.TableGraph(table, 0, 'cuda')
  ctx = contexts.NextStateTable(graph.table)

  def post():
    return nat.table_align_posteriors(graph, W, nf, lab, nl)

  def align():
    return nat.table_align(graph, W, nf, lab, nl)

  def loss_grad():
    return nat.table_loss_grad(graph, W, nf, lab, nl, True)

  def restate():
    return cpu.align_posteriors(W, nf.long(), lab, nl.long(), ctx, alignments.FrameDependent())

  nbytes = nat.ctypes.c_size_t(0)
  pb = nat._tproblem(graph, W, U)
  nat._check(nat.lib().lt_table_align_posteriors_workspace_bytes(
      nat.ctypes.byref(graph.g), nat.ctypes.byref(pb), nat.ctypes.byref(nbytes)), 'query')
  diff = float((post()[0] - restate()[0]).abs().max())
  (p_ms, a_ms, l_ms), spread = medians([post, align, loss_grad])
  r = sorted(batch_ms(restate, 1) for _ in range(RESTATE_CALLS))
  print(json.dumps({
      'workload': name, 'B': B, 'T': T, 'U': U, 'C': int(C), 'V': V,
      'dtype': str(dtype).split('.')[-1], 'align_post_ms': p_ms, 'align_ms': a_ms,
      'loss_grad_local_ms': l_ms, 'restatement_ms': statistics.median(r),
      'align_post_over_align': p_ms / a_ms, 'align_post_min_max_ms': spread[0],
      'align_min_max_ms': spread[1], 'loss_grad_local_min_max_ms': spread[2],
      'restatement_min_max_ms': (r[0], r[-1]), 'workspace_bytes': nbytes.value,
      'max_abs_diff': diff, 'batches': BATCHES, 'reps': REPS, 'settle_s': SETTLE_S,
      'device': torch.cuda.get_device_name(0)}), flush=True)


def main():
  if not torch.cuda.is_available():
    raise SystemExit('align_post_bench.py needs a ROCm GPU')
  only = os.environ.get('ONLY')
  if only in (None, 'bench'):
    run('FrameDependent x FullNGram bigram V=32 (bench shape)', 32, 1, 64, 1000, 100)
  if only in (None, 'bf16'):
    run('the bench shape, bf16 W', 32, 1, 64, 1000, 100, torch.bfloat16)


if __name__ == '__main__':
  main()
