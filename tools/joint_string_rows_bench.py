"""Times forced alignment on the rows a label string visits
(lt_joint_string_rows + lt_table_align / _long on the chain graph,
lt_joint_strings.hip) against the pair it replaces, lt_joint_weights_ex +
lt_table_align / _long on the model's graph, on the same inputs. Prints one
JSON line per workload (profiles/joint_string_rows_bench.jsonl keeps a run:
`python tools/joint_string_rows_bench.py > profiles/joint_string_rows_bench.jsonl`):

  rows_ms, align_chain_ms     _native.joint_string_rows; table_align on its rows
  weights_ms, align_model_ms  _native.joint_weights (fp32 W, split products);
                              table_align on it (bigram and trigram only: the
                              4-gram's W is 286 GB)
  ns_per_row                  rows_ms and weights_ms per formed row of V + 1
                              weights: B T (U+1) rows against B T C
  outputs_equal               the alignments of the two routes bit-equal
                              (asserted: the projections are N(0, 1))

The shape is bench.py's: B = 64, T = 1000, V = 32, H = 512, U in {100, 1000},
N(0, 1) projections, a blank bias of 3. A last line runs
RecognitionLattice.align and align_posteriors on the 4-gram at B = 64, U = 100
with lattice_fusion = 'on'.

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
from beam_joint_bench import NAMES, T, V, inputs  # noqa: E402

B, H = 64, 512


def run(n, graph, U):
  C = graph.C
  pc, pf, wo, bias = inputs(C, H, B)
  g = torch.Generator(device='cuda').manual_seed(U)
  nf = torch.full([B], T, dtype=torch.int32, device='cuda')
  lab = torch.randint(1, V + 1, [B, U], generator=g, device='cuda', dtype=torch.int32)
  nl = torch.full([B], U, dtype=torch.int32, device='cuda')
  chain = nat.chain_graph(U, V, 'cuda')
  align = nat.table_align if U <= 255 else nat.table_align_long
  if not nat.joint_string_rows_supported(graph, B, T, U, H):
    raise SystemExit(f'lt_joint_string_rows does not take H={H}, U={U}')
  held = {}

  def rows():
    held['Ws'] = nat.joint_string_rows(graph, pc, pf, wo, bias, nf, lab, nl)[0]

  def align_chain():
    return align(chain, held['Ws'], nf, lab, nl)

  def weights():
    held['W'] = nat.joint_weights(pc, pf, wo, bias)

  def align_model():
    return align(graph, held['W'], nf, lab, nl)

  pair = n < 3
  rows()
  fns = [rows, align_chain]
  equal = None
  if pair:
    weights()
    equal = all(torch.equal(a, b) for a, b in zip(align_chain(), align_model()))
    assert equal, 'the alignment on the rows must equal the alignment on W bit for bit'
    fns += [weights, align_model]
  med, spread = medians(fns)
  nrows, nW = B * T * (U + 1), B * T * C
  rec = {
      'workload': f'FullNGram {NAMES[n]} V={V}, H={H}, U={U}, forced alignment', 'B': B, 'T': T,
      'U': U, 'C': C, 'V': V, 'H': H, 'precision': 'fp32', 'rows_ms': med[0],
      'align_chain_ms': med[1], 'rows_min_max_ms': spread[0], 'align_chain_min_max_ms': spread[1],
      'rows_bytes': 4 * nrows * (V + 1), 'w_bytes': 4 * nW * (V + 1),
      'rows_ns_per_row': 1e6 * med[0] / nrows, 'outputs_equal': equal, 'batches': BATCHES,
      'reps': REPS, 'settle_s': SETTLE_S, 'device': torch.cuda.get_device_name(0)}
  if pair:
    rec.update(weights_ms=med[2], align_model_ms=med[3], weights_min_max_ms=spread[2],
               align_model_min_max_ms=spread[3], weights_ns_per_row=1e6 * med[2] / nW,
               route_over_pair=(med[0] + med[1]) / (med[2] + med[3]))
  print(json.dumps(rec), flush=True)


def api_fourgram(U=100):
  """RecognitionLattice.align / align_posteriors where W cannot exist."""
  context = lt.contexts.FullNGram(vocab_size=V, context_size=3)
  torch.manual_seed(0)
  lat = lt.RecognitionLattice(
      context=context, alignment=lt.alignments.FrameDependent(),
      weight_fn_cacher_factory=lambda c: lt.weight_fns.SharedEmbCacher(c.num_states(), 128,
                                                                       device='cuda'),
      weight_fn_factory=lambda c: lt.weight_fns.JointWeightFn(V, H, device='cuda',
                                                              lattice_fusion='on'))
  frames = torch.randn([B, T, 80], device='cuda')
  nf = torch.full([B], T, device='cuda')
  lab = torch.randint(1, V + 1, [B, U], device='cuda')
  nl = torch.full([B], U, device='cuda')
  ms = {}
  for name in ('align', 'align_posteriors'):
    fn = getattr(lat, name)
    fn(frames, nf, lab, nl)   # lazy layers, the graphs' device copies
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(frames, nf, lab, nl)
    torch.cuda.synchronize()
    ms[name] = 1e3 * (time.perf_counter() - t0)
    assert bool(torch.isfinite(out[-1]).all())
  print(json.dumps({
      'workload': f"RecognitionLattice.align / align_posteriors, FullNGram fourgram V={V}, "
                  f"H={H}, U={U}, lattice_fusion='on'", 'B': B, 'T': T, 'U': U,
      'C': context.num_states(), 'H': H, 'align_call_ms_host_clock': ms['align'],
      'align_posteriors_call_ms_host_clock': ms['align_posteriors'],
      'w_bytes': 4 * B * T * context.num_states() * (V + 1),
      'rows_bytes': 4 * B * T * (U + 1) * (V + 1),
      'device': torch.cuda.get_device_name(0)}), flush=True)


def main():
  if not torch.cuda.is_available():
    raise SystemExit('joint_string_rows_bench.py needs a ROCm GPU')
  only = os.environ.get('ONLY')
  for n in (1, 2, 3):
    if only not in (None, NAMES[n]):
      continue
    table = lt.contexts.FullNGram(vocab_size=V, context_size=n).next_state_table()
    graph = nat.TableGraph(table.to(torch.int32), 0, 'cuda')
    for U in (100, 1000):
      run(n, graph, U)
  if only in (None, 'api'):
    api_fourgram()


if __name__ == '__main__':
  main()
