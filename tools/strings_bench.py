"""Times the two kernels behind RecognitionLattice.string_weights / nbest_risk
(lt_table_strings_forward, lt_table_strings_backward: lt_strings.hip) against
the routes a user had before them. Prints one JSON line per workload and
appends it to OUT (default profiles/strings_bench.jsonl):

  forward_ms         lt_table_strings_forward alone: direction 0, scores only
  forward_hist_ms    the same with want_history: both directions and the
                     histories the backward reads
  backward_ms        lt_table_strings_backward alone: the dense fp32 dW
  per_hyp_ms         the route before: per hypothesis one lt_table_num_forward
                     (Log) and one lt_table_loss_grad (its gradient, as
                     _string_forward's backward runs it), N times on the same W
  torch_route_ms     cpu.string_scores forward + backward on the same ROCm
                     tensors: the definition in torch ops, a Python loop over
                     the frames
  workspace_bytes    lt_table_strings_workspace_bytes at the shape

The kernel timings: untimed calls for SETTLE_S seconds (default 1.0), then the
median over BATCHES (7) event-timed batches of REPS (10) calls, the kernels
alternating batch by batch. The two older routes take far longer a call: one
untimed call each, then the median of SLOW_CALLS (3) single timed calls run
between the kernels' batches. ONLY=fp32|bf16 and NS=4,16,64 select workloads.
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

SLOW_CALLS = int(os.environ.get('SLOW_CALLS', 3))
OUT = os.environ.get('OUT', os.path.join(ROOT, 'profiles', 'strings_bench.jsonl'))


def run(V, n, B, T, N, U, dtype):
  context = lt.contexts.FullNGram(vocab_size=V, context_size=n)
  table = context.next_state_table().to(torch.int32)
  C = table.shape[0]
  gen = torch.Generator(device='cuda')
  gen.manual_seed(0)
  W = torch.randn([B, T, C, V + 1], generator=gen, device='cuda').to(dtype)
  nf = torch.full([B], T, dtype=torch.int32, device='cuda')
  lab = torch.randint(1, V + 1, [B, N, U], generator=gen, device='cuda', dtype=torch.int32)
  nl = torch.randint(U // 2, U + 1, [B, N], generator=gen, device='cuda', dtype=torch.int32)
  grad = torch.randn([B, N], generator=gen, device='cuda')
  graph = nat.TableGraph(table, 0, 'cuda')
  pb = nat._tproblem(graph, W, U)
  ws_bytes = nat._workspace('lt_table_strings_workspace_bytes', graph, pb, W, N, alloc=False)[0]
  score, ws = nat.table_strings_forward(graph, W, nf, lab, nl, want_history=True)

  def forward():
    return nat.table_strings_forward(graph, W, nf, lab, nl)

  def forward_hist():
    return nat.table_strings_forward(graph, W, nf, lab, nl, want_history=True)

  def backward():
    return nat.table_strings_backward(graph, W, nf, lab, nl, score, grad, ws)

  def per_hyp():
    out = []
    for k in range(N):
      lk, nk = lab[:, k].contiguous(), nl[:, k].contiguous()
      out.append(nat.table_num_forward(graph, W, nf, lk, nk, nat.SEMIRING_LOG))
      nat.table_loss_grad(graph, W, nf, lk, nk, True)
    return torch.stack(out, 1)

  def torch_route():
    Wt = W.detach().float().requires_grad_(True)  # bf16 widened exactly
    s = cpu.string_scores(Wt, nf, lab, nl, lt.contexts.NextStateTable(graph.table))
    s.backward(grad)
    return s.detach(), Wt.grad

  # the routes agree before anything is timed (also the older routes' untimed calls)
  s_t, dW_t = torch_route()
  tol = 1e-4 * float(s_t.abs().max())
  assert torch.allclose(score, s_t, rtol=0, atol=tol)
  assert torch.allclose(per_hyp(), s_t, rtol=0, atol=tol)
  assert torch.allclose(backward(), dW_t, rtol=0, atol=1e-3 * float(grad.abs().max()))
  del s_t, dW_t
  kernels = {'forward': forward, 'forward_hist': forward_hist, 'backward': backward}
  slow = {'per_hyp': per_hyp, 'torch_route': torch_route}
  for fn in kernels.values():
    settle(fn)
  ms = {k: [] for k in (*kernels, *slow)}
  for i in range(BATCHES):
    for k, fn in kernels.items():
      ms[k].append(batch_ms(fn, REPS))
    if i < SLOW_CALLS:
      for k, fn in slow.items():
        ms[k].append(batch_ms(fn, 1))
  line = {'B': B, 'T': T, 'N': N, 'U': U, 'C': int(C), 'V': V,
          'dtype': str(dtype).split('.')[-1], 'workspace_bytes': int(ws_bytes)}
  line.update({f'{k}_ms': statistics.median(v) for k, v in ms.items()})
  line.update({f'{k}_min_max_ms': (min(v), max(v)) for k, v in ms.items()})
  line.update({'batches': BATCHES, 'reps': REPS, 'slow_calls': SLOW_CALLS, 'settle_s': SETTLE_S,
               'device': torch.cuda.get_device_name(0)})
  text = json.dumps(line)
  print(text, flush=True)
  os.makedirs(os.path.dirname(OUT), exist_ok=True)
  with open(OUT, 'a') as f:
    f.write(text + '\n')


def main():
  if not torch.cuda.is_available():
    raise SystemExit('strings_bench.py needs a ROCm GPU')
  only = os.environ.get('ONLY')
  for N in [int(x) for x in os.environ.get('NS', '4,16,64').split(',')]:
    if only in (None, 'fp32'):
      run(32, 1, 64, 1000, N, 100, torch.float32)
    if only in (None, 'bf16'):
      run(32, 1, 64, 1000, N, 100, torch.bfloat16)


if __name__ == '__main__':
  main()
