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

The long leg (ONLY=long; lt_table_align_expectation_long and
lt_table_string_scatter_long, lt_align_expect_long.hip) runs B=64, T=1000 at
U = 300, 600 and 1000, fp32 and bf16, one child process each, and APPENDS one
line per workload to profiles/align_expect_long_bench.jsonl: value_ms, full_ms,
scatter_ms and kernel_path_ms as above on the long calls, restatement_ms
(cpu.align_expectation on the device, value plus dW: the route such strings
took before the long kernels), restatement_over_kernel_path, and short_u255_ms,
the short kernel's full call on the first 255 labels of the same utterances,
with both kernels' microseconds per frame.

The parent process never touches the GPU: every workload runs in a child
process of its own under a time limit (CHILD_TIMEOUT_S, default 240), and a
child that fails or runs out of time ends the run -- nothing more is started
on the device after it.

Each kernel timing: untimed calls for SETTLE_S seconds (default 1.0; the clock
under load settles first, as bench.py does), then the median over BATCHES (7)
event-timed batches of REPS (10) calls; the kernels alternate batch by batch.
The restatement takes of the order of a second per call: one warm-up, then
the median of RESTATE_CALLS (3) single calls. ONLY=bench|bf16|long runs one
workload (long: its six).
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
OUT_LONG = os.path.join(ROOT, 'profiles', 'align_expect_long_bench.jsonl')
LONG_U = (300, 600, 1000)
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


def run_long(B, T, U, dtype):
  import torch
  from _timing import BATCHES, REPS, SETTLE_S, batch_ms, medians
  from last_torch_amd import _native as nat
  from last_torch_amd import alignments
  from last_torch_amd import contexts
  from last_torch_amd import cpu
  from last_torch_amd import lattices

  if not torch.cuda.is_available():
    raise SystemExit('align_expect_bench.py needs a ROCm GPU')
  V = 32
  dtype = getattr(torch, dtype)
  table = contexts.FullNGram(vocab_size=V, context_size=1).next_state_table().to(torch.int32)
  C = table.shape[0]
  g = torch.Generator(device='cuda')
  g.manual_seed(0)
  W = torch.randn([B, T, C, V + 1], generator=g, device='cuda').to(dtype)
  nf = torch.full([B], T, dtype=torch.int32, device='cuda')
  lab = torch.randint(1, V + 1, (B, U), generator=g, device='cuda', dtype=torch.int32)
  nl = torch.full([B], U, dtype=torch.int32, device='cuda')
  lv = torch.arange(T, dtype=torch.float32, device='cuda')[None, :, None].expand(B, T, U).contiguous()
  bv = torch.randn([B, T, U + 1], generator=g, device='cuda')
  ga = torch.randn([B], generator=g, device='cuda')
  gb = torch.randn([B], generator=g, device='cuda')
  lab_s, nl_s = lab[:, :255].contiguous(), torch.full_like(nl, 255)
  lv_s, bv_s = lv[:, :, :255].contiguous(), bv[:, :, :256].contiguous()
  graph = nat.TableGraph(table, 0, 'cuda')
  ctx = contexts.NextStateTable(graph.table)

  def value():
    return nat.table_align_expectation_long(graph, W, lv, bv, nf, lab, nl, want_post=False,
                                            want_cov=False)

  def full():
    return nat.table_align_expectation_long(graph, W, lv, bv, nf, lab, nl)

  cov = full()[4:]

  def scatter():
    return nat.table_string_scatter_long(graph, W, cov[0], cov[1], nf, lab, nl)

  def kernel_path():
    Wg = W.detach().requires_grad_(True)
    E, lp = lattices._AlignExpectFn.apply(Wg, lv, bv, nf, lab, nl, graph,
                                          lattices._AlignExpectFn.LONG_CALLS)
    (dW,) = torch.autograd.grad((ga * E + gb * lp).sum(), [Wg])
    return E, dW

  def short():
    return nat.table_align_expectation(graph, W, lv_s, bv_s, nf, lab_s, nl_s)

  def restate():
    Wg = W.detach().float().requires_grad_(True)
    E, lp = cpu.align_expectation(Wg, nf.long(), lab, nl.long(), ctx,
                                  alignments.FrameDependent(), lv, bv)
    (dW,) = torch.autograd.grad((ga * E + gb * lp).sum(), [Wg])
    return E.detach(), dW

  nbytes = nat.ctypes.c_size_t(0)
  pb = nat._tproblem(graph, W, U)
  nat._check(nat.lib().lt_table_align_expectation_long_workspace_bytes(
      nat.ctypes.byref(graph.g), nat.ctypes.byref(pb), nat.ctypes.byref(nbytes)), 'query')
  Ek, dWk = kernel_path()
  Er, dWr = restate()  # also the restatement's warm-up
  errs = {'max_abs_expected': float(Er.abs().max()), 'max_abs_dW': float(dWr.abs().max()),
          'diff_expected_kernel_path_vs_restatement': float((Ek.detach() - Er).abs().max()),
          'diff_dW_kernel_path_vs_restatement': float((dWk.float() - dWr).abs().max())}
  del Ek, dWk, Er, dWr
  (v_ms, f_ms, s_ms, k_ms, h_ms), spread = medians([value, full, scatter, kernel_path, short])
  r = sorted(batch_ms(restate, 1) for _ in range(RESTATE_CALLS))
  return {
      'workload': 'long strings, FrameDependent x FullNGram bigram V=32', 'B': B, 'T': T, 'U': U,
      'C': int(C), 'V': V, 'dtype': str(dtype).split('.')[-1], 'value_ms': v_ms, 'full_ms': f_ms,
      'scatter_ms': s_ms, 'kernel_path_ms': k_ms, 'short_u255_ms': h_ms,
      'restatement_ms': statistics.median(r),
      'restatement_over_kernel_path': statistics.median(r) / k_ms,
      'full_us_per_frame': 1e3 * f_ms / T, 'value_us_per_frame': 1e3 * v_ms / T,
      'short_u255_us_per_frame': 1e3 * h_ms / T, 'full_over_short_u255': f_ms / h_ms,
      'value_min_max_ms': spread[0], 'full_min_max_ms': spread[1],
      'scatter_min_max_ms': spread[2], 'kernel_path_min_max_ms': spread[3],
      'short_u255_min_max_ms': spread[4], 'restatement_min_max_ms': (r[0], r[-1]),
      'workspace_bytes': nbytes.value, **errs, 'batches': BATCHES, 'reps': REPS,
      'settle_s': SETTLE_S, 'device': torch.cuda.get_device_name(0)}


def child(*args):
  """One workload in a fresh process under its own time limit: its JSON line.
  A failure ends the run: nothing more is started on the device after it."""
  done = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', *args],
                        stdout=subprocess.PIPE, text=True, timeout=CHILD_TIMEOUT_S)
  if done.returncode != 0:
    raise SystemExit(f'workload {args!r} failed ({done.returncode}); nothing more is run')
  line = done.stdout.strip().splitlines()[-1]
  json.loads(line)
  print(line, flush=True)
  return line


def main():
  if len(sys.argv) == 3 and sys.argv[1] == '--child':  # one workload, on the GPU
    name, dtype = WORKLOADS[sys.argv[2]]
    print(json.dumps(run(name, 32, 1, 64, 1000, 100, dtype)), flush=True)
    return
  if len(sys.argv) == 5 and sys.argv[1:3] == ['--child', 'long']:
    print(json.dumps(run_long(64, 1000, int(sys.argv[3]), sys.argv[4])), flush=True)
    return
  only = os.environ.get('ONLY')
  lines = [child(key) for key in WORKLOADS if only in (None, key)]
  if only is None:
    with open(OUT, 'w') as f:
      f.write('\n'.join(lines) + '\n')
  if only in (None, 'long'):
    for U in LONG_U if 'LONG_U' not in os.environ else [int(os.environ['LONG_U'])]:
      for dtype in ('float32', 'bfloat16'):
        line = child('long', str(U), dtype)
        with open(OUT_LONG, 'a') as f:
          f.write(line + '\n')


if __name__ == '__main__':
  main()
