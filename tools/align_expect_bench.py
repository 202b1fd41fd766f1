"""Times the expectation over a transcript's alignments
(lt_table_align_expectation and lt_table_string_scatter, lt_align_expect.hip)
against its neighbours on the same inputs. Writes one JSON line per workload
to profiles/align_expect_bench.jsonl (and prints it):

  value_ms             _native.table_align_expectation, value-only: expected
                       and log_prob, no history, ends where the waves meet
  full_ms              the same call with emission, blank_occ, cov_lex and
                       cov_blank: what a forward that needs gradients runs
  scatter_ms           _native.table_string_scatter: the zeros over dW
                       [B,T,C,V+1] and the chain-head sums
  kernel_path_ms       value plus dW through autograd (_AlignExpectFn forward
                       and backward: full + the string-coordinate combination
                       + scatter + the cast to W's dtype)
  align_post_ms        _native.table_align_posteriors: the same two-wave
                       recursion without the means (the ratio full / align_post
                       is the cost of a frame step: both run nf steps per wave)
  align_ms             _native.table_align: the MaxTropical sibling
  restatement_ms       cpu.align_expectation on the device (double autograd
                       through the frame loop in torch ops), value plus dW: what
                       RecognitionLattice.align_expectation runs past the
                       kernel's range
  err_*                max abs error of `expected` and of dW against the
                       restatement run once in float64 (with their largest
                       magnitudes beside them): the kernel path's, and the
                       float32 restatement's on the same inputs

The parent process never touches the GPU: every workload runs in a child
process of its own under a time limit (CHILD_TIMEOUT_S, default 240), and a
child that fails or runs out of time ends the run -- nothing more is started
on the device after it.

Each kernel timing: untimed calls for SETTLE_S seconds (default 1.0; the clock
under load settles first, as bench.py does), then the median over BATCHES (7)
event-timed batches of REPS (10) calls; the kernels alternate batch by batch.
The restatement takes of the order of a second per call: one warm-up, then
the median of RESTATE_CALLS (3) single calls. ONLY=bench|bf16 runs one
workload.
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RESTATE_CALLS = int(os.environ.get('RESTATE_CALLS', 3))
CHILD_TIMEOUT_S = float(os.environ.get('CHILD_TIMEOUT_S', 240))
OUT = os.path.join(ROOT, 'profiles', 'align_expect_bench.jsonl')
WORKLOADS = {
    'bench': ('FrameDependent x FullNGram bigram V=32 (bench shape)', 'float32'),
    'bf16': ('the bench shape, bf16 W', 'bfloat16'),
}


def run(name, V, n, B, T, U, dtype):
  import torch
  from _timing import BATCHES, REPS, SETTLE_S, batch_ms, medians
  from last_torch_amd import _native as nat
  from last_torch_amd import alignments
  from last_torch_amd import contexts
  from last_torch_amd import cpu
  from last_torch_amd import lattices

  if not torch.cuda.is_available():
    raise SystemExit('align_expect_bench.py needs a ROCm GPU')
  dtype = getattr(torch, dtype)
  table = contexts.FullNGram(vocab_size=V, context_size=n).next_state_table().to(torch.int32)
  C = table.shape[0]
  g = torch.Generator(device='cuda')
  g.manual_seed(0)
  W = torch.randn([B, T, C, V + 1], generator=g, device='cuda').to(dtype)
  nf = torch.full([B], T, dtype=torch.int32, device='cuda')
  lab = torch.randint(1, V + 1, (B, U), generator=g, device='cuda', dtype=torch.int32)
  nl = torch.full([B], U, dtype=torch.int32, device='cuda')
  # expected emission delay: lexical_values[t, u] = t; a random blank term beside it
  lv = torch.arange(T, dtype=torch.float32, device='cuda')[None, :, None].expand(B, T, U).contiguous()
  bv = torch.randn([B, T, U + 1], generator=g, device='cuda')
  ga = torch.randn([B], generator=g, device='cuda')
  gb = torch.randn([B], generator=g, device='cuda')
  graph = nat.TableGraph(table, 0, 'cuda')
  ctx = contexts.NextStateTable(graph.table)

  def value():
    return nat.table_align_expectation(graph, W, lv, bv, nf, lab, nl, want_post=False,
                                       want_cov=False)

  def full():
    return nat.table_align_expectation(graph, W, lv, bv, nf, lab, nl)

  out = full()

  def scatter():
    return nat.table_string_scatter(graph, W, out[4], out[5], nf, lab, nl)

  def kernel_path():
    Wg = W.detach().requires_grad_(True)
    E, lp = lattices._AlignExpectFn.apply(Wg, lv, bv, nf, lab, nl, graph)
    (dW,) = torch.autograd.grad((ga * E + gb * lp).sum(), [Wg])
    return E, dW

  def post():
    return nat.table_align_posteriors(graph, W, nf, lab, nl)

  def align():
    return nat.table_align(graph, W, nf, lab, nl)

  def restate(dt=torch.float32):
    Wg = W.detach().to(dt).requires_grad_(True)
    E, lp = cpu.align_expectation(Wg, nf.long(), lab, nl.long(), ctx,
                                  alignments.FrameDependent(), lv, bv)
    (dW,) = torch.autograd.grad((ga.to(dt) * E + gb.to(dt) * lp).sum(), [Wg])
    return E.detach(), dW

  nbytes = nat.ctypes.c_size_t(0)
  pb = nat._tproblem(graph, W, U)
  nat._check(nat.lib().lt_table_align_expectation_workspace_bytes(
      nat.ctypes.byref(graph.g), nat.ctypes.byref(pb), nat.ctypes.byref(nbytes)), 'query')
  Ek, dWk = kernel_path()
  Er, dWr = restate()
  E64, dW64 = restate(torch.float64)
  errs = {'max_abs_expected': float(E64.abs().max()), 'max_abs_dW': float(dW64.abs().max()),
          'err_expected_kernel_path': float((Ek.detach().double() - E64).abs().max()),
          'err_expected_restatement_fp32': float((Er.double() - E64).abs().max()),
          'err_dW_kernel_path': float((dWk.double() - dW64).abs().max()),
          'err_dW_restatement_fp32': float((dWr.double() - dW64).abs().max())}
  del Er, dWr, dWk, E64, dW64
  (v_ms, f_ms, s_ms, k_ms, p_ms, a_ms), spread = medians(
      [value, full, scatter, kernel_path, post, align])
  r = sorted(batch_ms(restate, 1) for _ in range(RESTATE_CALLS))
  return {
      'workload': name, 'B': B, 'T': T, 'U': U, 'C': int(C), 'V': V,
      'dtype': str(dtype).split('.')[-1], 'value_ms': v_ms, 'full_ms': f_ms, 'scatter_ms': s_ms,
      'kernel_path_ms': k_ms, 'align_post_ms': p_ms, 'align_ms': a_ms,
      'restatement_ms': statistics.median(r), 'full_over_align_post': f_ms / p_ms,
      'value_over_align_post': v_ms / p_ms,
      'restatement_over_kernel_path': statistics.median(r) / k_ms,
      'value_min_max_ms': spread[0], 'full_min_max_ms': spread[1],
      'scatter_min_max_ms': spread[2], 'kernel_path_min_max_ms': spread[3],
      'align_post_min_max_ms': spread[4], 'align_min_max_ms': spread[5],
      'restatement_min_max_ms': (r[0], r[-1]), 'workspace_bytes': nbytes.value,
      **errs, 'batches': BATCHES, 'reps': REPS, 'settle_s': SETTLE_S,
      'device': torch.cuda.get_device_name(0)}


def main():
  if len(sys.argv) == 3 and sys.argv[1] == '--child':  # one workload, on the GPU
    name, dtype = WORKLOADS[sys.argv[2]]
    print(json.dumps(run(name, 32, 1, 64, 1000, 100, dtype)), flush=True)
    return
  only = os.environ.get('ONLY')
  lines = []
  for key in WORKLOADS:
    if only not in (None, key):
      continue
    # a fresh process per workload, under its own time limit; a failure ends the run
    done = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', key],
                          stdout=subprocess.PIPE, text=True, timeout=CHILD_TIMEOUT_S)
    if done.returncode != 0:
      raise SystemExit(f'workload {key!r} failed ({done.returncode}); nothing more is run')
    line = done.stdout.strip().splitlines()[-1]
    json.loads(line)
    print(line, flush=True)
    lines.append(line)
  if only is None:
    with open(OUT, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
