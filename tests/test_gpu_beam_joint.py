"""GPU tests of lt_joint_beam_search (lt_beam_joint.hip, include/lt_beam_joint.h):
prefix beam search with JointWeightFn's arc weights formed inside the search.

1. Bit for bit what lt_table_beam_search returns on lt_joint_weights_ex's fp32
   W (the two entry points the fused one replaces), in both semirings, over the
   shapes at which the kernel takes another path.
2. Exactly cpu.beam_search on weights every sum of which is exact (tanh = +-1,
   eighths): the total order over heavy ties, independent of the producer.
3. Nothing pruned (V = 2, T = 4, K = 32): every hypothesis' Log score against
   the float64 string forward, within T times the producer tests' per-element
   bound for split products (test_gpu_producer._tol32), on the split and on
   the direct (|frame_proj| > 40) path.
4. RecognitionLattice.beam_search: lattice_fusion 'on' equals 'off'.
5. Return codes with nothing launched, poisoned / stale buffers, a captured
   graph.
"""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

import last_torch_amd as lt
from last_torch_amd import _native as nat
from last_torch_amd import cpu
from poisoned_buffers import poisoned, stale
import sample_ref
import test_gpu_producer as producer

pytestmark = pytest.mark.gpu

SIDS = {'Log': nat.SEMIRING_LOG, 'MaxTropical': nat.SEMIRING_MAX}
_bigram32 = lambda rng: lt.contexts.FullNGram(vocab_size=32, context_size=1)
# name: (context, H, K, T, precision)
CASES = {
    'ring_tail': (_bigram32, 64, 16, 70, 'fp32'),        # T no multiple of the frame ring
    'two_row_tiles': (_bigram32, 64, 64, 24, 'bf16'),
    'greedy_one_kstep': (_bigram32, 16, 1, 40, 'fp32'),
    'odd_ksteps': (_bigram32, 48, 40, 24, 'fp32'),       # second row tile partly live
    'two_col_tiles': (lambda rng: lt.contexts.NextStateTable(sample_ref.random_table(rng, 5, 40)),
                      32, 8, 12, 'fp32'),                # R = 41
    'gathered_table': (lambda rng: lt.contexts.FullNGram(vocab_size=8, context_size=3),
                       32, 8, 30, 'fp32'),               # C = 585: e^{2 ctx_proj} stays in memory
    'short_ring_h512': (_bigram32, 512, 8, 11, 'fp32'),  # e^{2 ctx_proj} in LDS, 2-frame slices
}


def _inputs(device, C, R, H, B, T, seed):
  """N(0, 1) projections (all within +-40), a blank bias so that prefixes stay
  in the beam beside their parents and the merge matters."""
  g = torch.Generator(device=device)
  g.manual_seed(seed)
  pc = torch.randn([C, H], generator=g, device=device)
  pf = torch.randn([B, T, H], generator=g, device=device)
  wo = torch.randn([R, H], generator=g, device=device) / H ** 0.5
  bias = torch.randn([R], generator=g, device=device)
  bias[0] += 2.0
  return pc, pf, wo, bias


@functools.lru_cache(maxsize=None)
def _case(name, device):
  make, H, K, T, precision = CASES[name]
  context = make(np.random.default_rng(sum(map(ord, name))))
  table = sample_ref.table_of(context)
  graph = nat.TableGraph(table, 0, device)
  ops = _inputs(device, graph.C, graph.V + 1, H, 4, T, seed=len(name))
  nf = torch.tensor([T, T - 3, 1, 0], dtype=torch.int32, device=device)
  return graph, ops, nf, K, precision


def _bits(t):
  return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize('semiring', list(SIDS))
@pytest.mark.parametrize('name', list(CASES))
def test_bit_equal_to_the_materialised_path(cuda, name, semiring):
  graph, ops, nf, K, precision = _case(name, cuda)
  assert float(max(ops[0].abs().max(), ops[1].abs().max())) <= 40
  W = nat.joint_weights(*ops, precision=precision)
  want = nat.table_beam_search(graph, W, nf, K, SIDS[semiring], want_trace=True)
  got = nat.joint_beam_search(graph, *ops, nf, K, SIDS[semiring], precision, want_trace=True)
  torch.cuda.synchronize()
  assert int((want[2][0] > -np.inf).sum()) == K   # a filled beam
  for g, w in zip(got, want):
    assert g.dtype == w.dtype and torch.equal(_bits(g), _bits(w))


@pytest.mark.parametrize('K', [4, 64])
def test_exact_against_the_host_definition(cuda, K):
  V, H, T, B = 32, 64, 24, 4
  context = lt.contexts.FullNGram(vocab_size=V, context_size=1)
  g = torch.Generator().manual_seed(K)
  sign = lambda shape: torch.randint(0, 2, shape, generator=g).double() * 2 - 1
  eighths = lambda shape: torch.randint(-16, 17, shape, generator=g).double() / 8
  pc, pf = 20 * sign([V + 1, H]), 4 * sign([B, T, H])
  wo, bias = eighths([V + 1, H]), eighths([V + 1])
  # |x| >= 16: tanh is +-1 in fp32 (the kernel's and the host's), and within
  # 2^-44 of it in float64, where the plain formula is then off an exact W by
  # rounding dust only: W is formed from the rounded hidden values
  hid = torch.tanh(pc[None, None] + pf[:, :, None])
  assert float((hid.abs() - 1).abs().max()) < 2.0 ** -44
  W64 = hid.round() @ wo.t() + bias
  assert float((hid @ wo.t() + bias - W64).abs().max()) < 1e-10
  W = W64.float()
  assert torch.equal(W.double(), W64)   # the cast is lossless: every sum is exact
  nf = torch.tensor([T, T - 3, 1, 0])
  want = cpu.beam_search(W, nf, context, K, lt.semirings.MaxTropical)
  graph = nat.TableGraph(context.next_state_table(), 0, cuda)
  got = nat.joint_beam_search(graph, *(x.float().to(cuda) for x in (pc, pf, wo, bias)),
                              nf.int().to(cuda), K, nat.SEMIRING_MAX)
  assert len({float(x) for x in W[0, 0].flatten()}) < W[0, 0].numel() // 2   # W is full of ties
  for g_, w in zip(got, want):
    assert torch.equal(g_.cpu().long() if g_.dtype == torch.int32 else g_.cpu(), w)


@pytest.mark.parametrize('over40', [False, True])
def test_nothing_pruned_against_float64(cuda, over40):
  V, T, K, H = 2, 4, 32, 32
  context = lt.contexts.FullNGram(vocab_size=V, context_size=1)
  table = sample_ref.table_of(context)
  pc, pf, wo, bias = _inputs(cuda, V + 1, V + 1, H, 1, T, seed=7)
  if over40:
    pf[:, 1::2] *= 30.0   # frames 1 and 3 take the direct path
    assert float(pf[0, 1].abs().max()) > 40 and float(pf[0, 0].abs().max()) <= 40
  tol = T * float(producer._tol32(pc, pf, wo).max())
  W64 = (torch.tanh(pc.double()[None] + pf.double()[0, :, None]) @ wo.double().t() +
         bias.double()).cpu().numpy()   # [T, C, V+1]
  forward = {}   # label sequence -> float64 logsumexp over its alignments
  for path in itertools.product(range(V + 1), repeat=T):
    seq = tuple(y for y in path if y)
    forward[seq] = np.logaddexp(forward.get(seq, -np.inf), sample_ref.path_weight(W64, path, table)[0])
  assert len(forward) == 31
  graph = nat.TableGraph(table, 0, cuda)
  nf = torch.tensor([T], dtype=torch.int32, device=cuda)
  labels, nl, scores = (x.cpu() for x in nat.joint_beam_search(graph, pc, pf, wo, bias, nf, K,
                                                                nat.SEMIRING_LOG))
  live = torch.isfinite(scores[0])
  assert int(live.sum()) == 31 and bool(live[:31].all())
  got = {tuple(labels[0, r, :nl[0, r]].tolist()): float(scores[0, r]) for r in range(31)}
  assert set(got) == set(forward)
  for seq, s in got.items():
    assert abs(s - forward[seq]) <= tol, (seq, s, forward[seq], tol)
  log_z = np.logaddexp.reduce(list(forward.values()))
  assert abs(float(torch.logsumexp(scores[0, :31].double(), 0)) - log_z) <= tol


def test_public_interface_on_equals_off(cuda, monkeypatch):
  V, H, B, T, K = 32, 64, 3, 20, 8
  torch.manual_seed(3)
  context = lt.contexts.FullNGram(vocab_size=V, context_size=1)
  lat = lt.RecognitionLattice(
      context=context, alignment=lt.alignments.FrameDependent(),
      weight_fn_cacher_factory=lambda c: lt.weight_fns.SharedEmbCacher(c.num_states(), 16,
                                                                       device=cuda),
      weight_fn_factory=lambda c: lt.weight_fns.JointWeightFn(V, H, device=cuda))
  frames = torch.randn([B, T, 24], device=cuda)
  nf = torch.tensor([T, T - 3, 0], device=cuda)
  calls = []
  real = nat.joint_beam_search
  monkeypatch.setattr(nat, 'joint_beam_search', lambda *a, **k: calls.append(1) or real(*a, **k))
  out = {}
  for fusion in ('off', 'on', 'auto'):
    lat.weight_fn.lattice_fusion = fusion
    out[fusion] = lat.beam_search(frames, nf, K, lt.semirings.Log)
    assert len(calls) == (fusion != 'off')   # 'auto': W fits in memory, so it is materialised
  labels, nl, scores = out['on']
  assert labels.dtype == torch.int64 and tuple(labels.shape) == (B, K, T)
  assert nl.dtype == torch.int64 and tuple(nl.shape) == (B, K)
  assert scores.dtype == torch.float32 and tuple(scores.shape) == (B, K)
  assert int(nl[0, 0]) > 0 and not scores.requires_grad
  for a, b in zip(out['on'], out['off']):
    assert torch.equal(_bits(a), _bits(b))


def test_abi_error_codes(cuda):
  """LT_EINVAL and LT_EUNSUPPORTED as include/lt_beam_joint.h lists them;
  nothing is launched, so the outputs stay untouched."""
  lib = nat.lib()
  V, T, B, K, H = 4, 6, 2, 3, 32
  context = lt.contexts.FullNGram(vocab_size=V, context_size=1)
  graph = nat.TableGraph(context.next_state_table(), 0, cuda)
  fld = nat.TableGraph(context.next_state_table(), 1, cuda)
  wide = nat.TableGraph(lt.contexts.FullNGram(vocab_size=64, context_size=1).next_state_table(),
                        0, cuda)
  ops = _inputs(cuda, V + 1, V + 1, H, B, T, seed=1)
  nf = torch.tensor([T, 4], dtype=torch.int32, device=cuda)
  labels = torch.full([B, 65, T], -7, dtype=torch.int64, device=cuda)
  nl = torch.full([B, 65], -7, dtype=torch.int32, device=cuda)
  scores = torch.full([B, 65], -7.0, device=cuda)
  trace = torch.full([B, T, 65], -7, dtype=torch.int32, device=cuda)
  step = torch.full([B, T, 65], -7.0, device=cuda)
  ws = torch.empty([1 << 16], dtype=torch.float32, device=cuda)
  ptr = nat._ptr

  def both(g=graph, beam=K, sid=nat.SEMIRING_LOG, lab=labels, ws=ws, hidden=H, pc=ops[0],
           dtype=nat.LT_DTYPE_F32, precision=nat.JOINT_SPLIT):
    pb = nat.TableProblem(B, T, 0, dtype)
    jp = nat.JointParams(hidden, precision, *(None if x is None else x.data_ptr()
                                              for x in (pc, ops[1].reshape(-1, H), *ops[2:])))
    query = lib.lt_joint_beam_search_workspace_bytes(
        ctypes.byref(g.g), ctypes.byref(pb), ctypes.byref(jp), beam,
        ctypes.byref(ctypes.c_size_t(0)))
    call = lib.lt_joint_beam_search(
        ctypes.byref(g.g), ctypes.byref(pb), ctypes.byref(jp), ptr(nf), beam, sid, ptr(lab),
        ptr(nl), ptr(scores), ptr(trace), ptr(step), ptr(ws), ws.numel() * 4 if ws is not None else 0,
        nat._stream())
    return call, query

  assert both(beam=0) == (-1, -1)
  assert both(precision=7) == (-1, -1)
  for kw in (dict(sid=nat.SEMIRING_REAL), dict(lab=None), dict(pc=None), dict(ws=None)):
    assert both(**kw) == (-1, 0), kw
  for kw in (dict(g=fld), dict(beam=65), dict(g=wide), dict(hidden=24),
             dict(dtype=nat.LT_DTYPE_BF16),
             dict(hidden=1024, g=nat.TableGraph(torch.zeros([2, 63], dtype=torch.int32), 0, cuda))):
    assert both(**kw) == (nat.LT_EUNSUPPORTED, nat.LT_EUNSUPPORTED), kw   # the last: 264 KB of LDS
  torch.cuda.synchronize()
  for t in (labels, nl, trace):
    assert (t == -7).all()
  assert (scores == -7).all() and (step == -7).all()
  assert nat.joint_beam_search_supported(graph, B, T, H, K)
  assert not nat.joint_beam_search_supported(graph, B, T, H, 65)


@pytest.mark.parametrize('mode', ['poisoned', 'stale'])
@pytest.mark.parametrize('want_trace', [True, False])
def test_poisoned_and_stale_buffers(cuda, mode, want_trace):
  """Every output element and every workspace byte read is written by the
  call: on 0xFF-filled buffers, and on the buffers a finished call on other
  projections (over 40: every flag set) left, the bits are a plain run's."""
  graph, (pc, pf, wo, bias), nf, K, precision = _case('ring_tail', cuda)
  fn = lambda x: nat.joint_beam_search(graph, x[0], x[1], wo, bias, x[2], K, nat.SEMIRING_LOG,
                                       precision, want_trace=want_trace)
  plain = [t.clone() for t in fn((pc, pf, nf))]
  rerun = fn((pc, pf, nf))
  for p, r in zip(plain, rerun):
    assert torch.equal(_bits(p), _bits(r))
  if mode == 'poisoned':
    with poisoned(nat):
      out = fn((pc, pf, nf))
  else:
    with stale(nat) as s:
      s.record(fn, (pc * 100, pf.flip(0), nf.flip(0)))
      torch.cuda.synchronize()
      out = s.replay(fn, (pc, pf, nf))
  torch.cuda.synchronize()
  assert len(out) == len(plain) == (5 if want_trace else 3)
  for p, o in zip(plain, out):
    assert torch.equal(p.view(torch.uint8), o.view(torch.uint8))


def test_graph_replays_match_eager(cuda):
  """Both launches captured on one stream and replayed on new projections
  equal eager calls, replay after replay."""
  graph, ops, nf, K, precision = _case('ring_tail', cuda)
  pc, pf, wo, bias = (x.clone() for x in ops)
  B, T, H = pf.shape
  jp, keep = nat._joint(pc, pf, wo, bias, precision)
  assert keep[0].data_ptr() == pc.data_ptr() and keep[1].data_ptr() == pf.data_ptr()
  pb = nat.TableProblem(B, T, 0, nat.LT_DTYPE_F32)
  labels = torch.empty([B, K, T], dtype=torch.int64, device=cuda)
  nl = torch.empty([B, K], dtype=torch.int32, device=cuda)
  scores = torch.empty([B, K], device=cuda)
  ws = torch.empty([256 + graph.C * H + B * T * K], dtype=torch.float32, device=cuda)

  def call():
    nat._check(nat.lib().lt_joint_beam_search(
        ctypes.byref(graph.g), ctypes.byref(pb), ctypes.byref(jp), nat._ptr(nf), K,
        nat.SEMIRING_LOG, nat._ptr(labels), nat._ptr(nl), nat._ptr(scores), None, None,
        nat._ptr(ws), ws.numel() * 4, nat._stream()), 'lt_joint_beam_search')

  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(s):
    call()  # eager on the side stream first, as torch's capture recipe does
  torch.cuda.current_stream().wait_stream(s)
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    call()
  for seed in (2, 3, 4):
    pc2, pf2, _, _ = _inputs(cuda, graph.C, graph.V + 1, H, B, T, seed)
    pc.copy_(pc2 * (50 if seed == 4 else 1))   # the last replay: the over-40 flags change
    pf.copy_(pf2)
    g.replay()
    torch.cuda.synchronize()
    want = nat.joint_beam_search(graph, pc, pf, wo, bias, nf, K, nat.SEMIRING_LOG, precision)
    for got, w in zip((labels, nl, scores), want):
      assert torch.equal(_bits(got), _bits(w))
