"""GPU tests of lt_joint_string_rows (lt_joint_strings.hip,
include/lt_joint_strings.h): the rows of JointWeightFn's arc weights that a
label string visits, formed without W.

1. Bit for bit lt_joint_weights_ex's rows W[b, t, states[b, k]] on live
   elements, exactly 0 elsewhere, states against a plain walk of the table,
   over the shapes at which the kernels take another path.
2. The fp32 split rows against bias + tanh(pc[s_k] + pf) @ wo.T in float64,
   within the producer tests' per-element bound (test_gpu_producer._tol32), on
   the split and on the direct (|frame_proj| > 40) path.
3. RecognitionLattice.align / align_posteriors: lattice_fusion 'on' equals
   'off' bit for bit, short and long kernels, an utterance without a path.
4. Return codes with nothing launched, poisoned / stale buffers, a captured
   graph.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import last_torch_amd as lt
from last_torch_amd import _native as nat
from poisoned_buffers import poisoned, stale
import sample_ref
from test_gpu_beam_joint import _bits, _inputs
import test_gpu_producer as producer

pytestmark = pytest.mark.gpu

_bigram32 = lambda rng: lt.contexts.FullNGram(vocab_size=32, context_size=1)
F32, BF16 = torch.float32, torch.bfloat16
# name: (context, H, U, T, precision, dtype of the rows)
CASES = {
    'second_tile_partly_live': (_bigram32, 64, 40, 12, 'fp32', F32),
    'one_full_tile': (_bigram32, 64, 31, 12, 'fp32', F32),
    'slice_tail': (_bigram32, 32, 70, 37, 'fp32', F32),   # T no multiple of the frame slice
    'one_kstep': (_bigram32, 16, 40, 12, 'fp32', F32),
    'odd_ksteps': (_bigram32, 48, 40, 12, 'fp32', F32),
    'h512': (_bigram32, 512, 40, 12, 'fp32', F32),
    'h784': (_bigram32, 784, 40, 12, 'fp32', F32),         # context rows read from the workspace
    'two_col_tiles': (lambda rng: lt.contexts.NextStateTable(sample_ref.random_table(rng, 5, 40)),
                      32, 40, 12, 'fp32', F32),            # R = 41
    'gathered_context': (lambda rng: lt.contexts.FullNGram(vocab_size=8, context_size=3),
                         32, 40, 12, 'fp32', F32),         # C = 585
    'bf16_products': (_bigram32, 64, 40, 12, 'bf16', F32),
    'bf16_rows': (_bigram32, 64, 40, 12, 'fp32', BF16),
}


def _labels(rng, V, U, device):
  """[4, U]: all labels; epsilons (0 and a value > V) inside and past
  num_labels; labels with num_labels = 0; mostly epsilons."""
  lab = rng.integers(1, V + 1, [4, U])
  lab[1, 2::5], lab[1, 3::7] = 0, V + 5
  lab[3, 2:] = np.where(rng.random(U - 2) < 0.8, 0, lab[3, 2:])
  nl = [U, U - 6, 0, 3]
  return (torch.tensor(lab, dtype=torch.int32, device=device),
          torch.tensor(nl, dtype=torch.int32, device=device))


@functools.lru_cache(maxsize=None)
def _case(name, device):
  make, H, U, T, precision, dtype = CASES[name]
  rng = np.random.default_rng(sum(map(ord, name)))
  table = sample_ref.table_of(make(rng))
  graph = nat.TableGraph(table, 0, device)
  ops = _inputs(device, graph.C, graph.V + 1, H, 4, T, seed=len(name))
  nf = torch.tensor([T, T - 3, 1, 0], dtype=torch.int32, device=device)
  lab, nl = _labels(rng, graph.V, U, device)
  return graph, table, ops, nf, lab, nl, precision, dtype


def _walk(table, lab):
  """states [B, U+1] (-1 past n_b) by a plain walk of the table."""
  B, U = lab.shape
  V = table.shape[1]
  out = np.full([B, U + 1], -1, np.int32)
  for b in range(B):
    c, k = 0, 0
    out[b, 0] = 0
    for y in lab[b]:
      if 1 <= y <= V:
        c = int(table[c, y - 1])
        k += 1
        out[b, k] = c
  return out


@pytest.mark.parametrize('name', list(CASES))
def test_bit_equal_to_the_materialised_rows(cuda, name):
  graph, table, ops, nf, lab, nl, precision, dtype = _case(name, cuda)
  assert float(max(ops[0].abs().max(), ops[1].abs().max())) <= 40
  W = nat.joint_weights(*ops, dtype=dtype, precision=precision)
  Ws, states = nat.joint_string_rows(graph, *ops, nf, lab, nl, precision, dtype)
  torch.cuda.synchronize()
  want_states = _walk(table, lab.cpu().numpy())
  assert np.array_equal(states.cpu().numpy(), want_states)
  assert (want_states[0] >= 0).all() and (want_states[3] < 0).any()
  want = torch.zeros_like(Ws)
  for b in range(4):
    n = int((want_states[b] >= 0).sum())
    f = int(nf[b])
    want[b, :f, :n] = W[b, :f, torch.tensor(want_states[b, :n], device=cuda).long()]
  assert Ws.dtype == dtype and torch.equal(Ws.view(torch.uint8), want.view(torch.uint8))


@pytest.mark.parametrize('over40', [False, True])
def test_against_float64(cuda, over40):
  graph, table, (pc, pf, wo, bias), nf, lab, nl, _, _ = _case('second_tile_partly_live', cuda)
  if over40:
    pf = pf.clone()
    pf[:, 1] *= 30.0   # frame 1 takes the direct path
    assert float(pf[0, 1].abs().max()) > 40 and float(pf[0, 0].abs().max()) <= 40
  Ws, states = nat.joint_string_rows(graph, pc, pf, wo, bias, nf, lab, nl)
  for b in range(4):
    n, f = int((states[b] >= 0).sum()), int(nf[b])
    rows = pc[states[b, :n].long()]
    ref = (torch.tanh(rows.double()[None] + pf[b, :f].double()[:, None]) @ wo.double().t() +
           bias.double())
    err = (Ws[b, :f, :n].double() - ref).abs()
    tol = producer._tol32(rows, pf[b, :f], wo)
    print(f'over40={over40} b={b}: max err {float(err.max()) if f else 0:.3e}, '
          f'min tol {float(tol.min()) if f else 0:.3e}')
    assert bool((err <= tol).all())


def _lattice(V, H, device):
  torch.manual_seed(5)
  return lt.RecognitionLattice(
      context=lt.contexts.FullNGram(vocab_size=V, context_size=1),
      alignment=lt.alignments.FrameDependent(),
      weight_fn_cacher_factory=lambda c: lt.weight_fns.SharedEmbCacher(c.num_states(), 16,
                                                                       device=device),
      weight_fn_factory=lambda c: lt.weight_fns.JointWeightFn(V, H, device=device))


# V, H, U, T, num_frames, num_labels
END_TO_END = {
    'short_kernels': (32, 64, 20, 30, [30, 27, 0], [20, 12, 0]),
    'long_kernels': (8, 16, 260, 280, [280, 270], [260, 200]),
    'no_path': (32, 64, 20, 12, [12, 12], [20, 8]),   # utterance 0: num_labels > T
}


@pytest.mark.parametrize('name', list(END_TO_END))
def test_public_interface_on_equals_off(cuda, monkeypatch, name):
  V, H, U, T, nf, nl = END_TO_END[name]
  B = len(nf)
  lat = _lattice(V, H, cuda)
  g = torch.Generator().manual_seed(U)
  frames = torch.randn([B, T, 24], generator=g).to(cuda)
  labels = torch.randint(1, V + 1, [B, U], generator=g).to(cuda)
  labels[-1, 3] = 0   # an epsilon inside the string
  nf, nl = torch.tensor(nf, device=cuda), torch.tensor(nl, device=cuda)
  calls = []
  real = nat.joint_string_rows
  monkeypatch.setattr(nat, 'joint_string_rows', lambda *a, **k: calls.append(1) or real(*a, **k))
  out = {}
  for fusion in ('off', 'on', 'auto'):
    lat.weight_fn.lattice_fusion = fusion
    out[fusion] = (lat.align(frames, nf, labels, nl) +
                   lat.align_posteriors(frames, nf, labels, nl))
    assert len(calls) == (2 if fusion != 'off' else 0)   # 'auto': W fits, so it is materialised
  for a, b in zip(out['on'], out['off']):
    assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))
  path, label_frames, weight, emission, log_prob = out['on']
  if name == 'no_path':
    assert not path[0].any() and (label_frames[0] == -1).all() and not emission[0].any()
    assert float(weight[0]) == float(log_prob[0]) == -np.inf
  assert bool(torch.isfinite(weight[1])) and int((label_frames[1] >= 0).sum()) > 0


def test_abi_error_codes(cuda):
  """LT_EINVAL and LT_EUNSUPPORTED as include/lt_joint_strings.h lists them;
  nothing is launched, so the outputs stay untouched."""
  lib = nat.lib()
  V, T, B, U, H = 4, 6, 2, 5, 32
  table = lt.contexts.FullNGram(vocab_size=V, context_size=1).next_state_table()
  graph, fld = nat.TableGraph(table, 0, cuda), nat.TableGraph(table, 1, cuda)
  wide = nat.TableGraph(lt.contexts.FullNGram(vocab_size=64, context_size=1).next_state_table(),
                        0, cuda)
  ops = _inputs(cuda, V + 1, V + 1, H, B, T, seed=1)
  nf = torch.tensor([T, 4], dtype=torch.int32, device=cuda)
  lab = torch.ones([B, 4096], dtype=torch.int32, device=cuda)
  Ws = torch.full([B * T * 4097 * 65], -7.0, device=cuda)
  states = torch.full([B, 4097], -7, dtype=torch.int32, device=cuda)
  ws = torch.empty([1 << 22], dtype=torch.float32, device=cuda)
  ptr = nat._ptr

  def both(g=graph, U=U, lab=lab, ws=ws, hidden=H, pc=ops[0], pf=ops[1].reshape(-1, H),
           dtype=nat.LT_DTYPE_F32, precision=nat.JOINT_SPLIT):
    pb = nat.TableProblem(B, T, U, dtype)
    jp = nat.JointParams(hidden, precision, *(None if x is None else x.data_ptr()
                                              for x in (pc, pf, *ops[2:])))
    query = lib.lt_joint_string_rows_workspace_bytes(
        ctypes.byref(g.g), ctypes.byref(pb), ctypes.byref(jp), ctypes.byref(ctypes.c_size_t(0)))
    call = lib.lt_joint_string_rows(
        ctypes.byref(g.g), ctypes.byref(pb), ctypes.byref(jp), ptr(nf), ptr(lab), None, ptr(Ws),
        ptr(states), ptr(ws), ws.numel() * 4 if ws is not None else 0, nat._stream())
    return call, query

  for kw in (dict(precision=7), dict(dtype=5), dict(hidden=0)):
    assert both(**kw) == (-1, -1), kw
  for kw in (dict(lab=None), dict(pc=None), dict(ws=None), dict(ws=ws[:8]),
             dict(pf=ops[1].reshape(-1)[1:])):   # the last: frame_proj 4 bytes off 16
    assert both(**kw) == (-1, 0), kw
  for kw in (dict(g=fld), dict(g=wide), dict(hidden=24), dict(hidden=1040), dict(U=0),
             dict(U=4096),
             dict(hidden=1024, g=nat.TableGraph(torch.zeros([2, 63], dtype=torch.int32), 0, cuda))):
    assert both(**kw) == (nat.LT_EUNSUPPORTED, nat.LT_EUNSUPPORTED), kw   # the last: 280 KB of LDS
  torch.cuda.synchronize()
  assert (Ws == -7).all() and (states == -7).all()
  assert nat.joint_string_rows_supported(graph, B, T, U, H)
  assert not nat.joint_string_rows_supported(graph, B, T, 4096, H)


@pytest.mark.parametrize('mode', ['poisoned', 'stale'])
def test_poisoned_and_stale_buffers(cuda, mode):
  """Every element of Ws and states and every workspace byte read is written
  by the call: on 0xFF-filled buffers, and on the buffers a finished call on
  other inputs (over 40: the flags set, other strings) left, the bits are a
  plain run's."""
  graph, _, (pc, pf, wo, bias), nf, lab, nl, precision, dtype = _case('slice_tail', cuda)
  fn = lambda x: nat.joint_string_rows(graph, x[0], x[1], wo, bias, x[2], x[3], nl, precision,
                                       dtype)
  plain = [t.clone() for t in fn((pc, pf, nf, lab))]
  for p, r in zip(plain, fn((pc, pf, nf, lab))):
    assert torch.equal(_bits(p), _bits(r))
  if mode == 'poisoned':
    with poisoned(nat):
      out = fn((pc, pf, nf, lab))
  else:
    with stale(nat) as s:
      s.record(fn, (pc * 100, pf.flip(0), nf.flip(0), lab.flip(0).contiguous()))
      torch.cuda.synchronize()
      out = s.replay(fn, (pc, pf, nf, lab))
  torch.cuda.synchronize()
  for p, o in zip(plain, out):
    assert torch.equal(p.view(torch.uint8), o.view(torch.uint8))


def test_graph_replays_match_eager(cuda):
  """Both launches captured on one stream and replayed on new projections
  equal eager calls, replay after replay."""
  graph, _, ops, nf, lab, nl, precision, dtype = _case('slice_tail', cuda)
  pc, pf, wo, bias = (x.clone() for x in ops)
  B, T, H = pf.shape
  U = lab.shape[1]
  jp, keep = nat._joint(pc, pf, wo, bias, precision)
  assert keep[0].data_ptr() == pc.data_ptr() and keep[1].data_ptr() == pf.data_ptr()
  pb = nat.TableProblem(B, T, U, nat.LT_DTYPE_F32)
  Ws = torch.empty([B, T, U + 1, graph.V + 1], device=cuda)
  states = torch.empty([B, U + 1], dtype=torch.int32, device=cuda)
  ws = torch.empty([1024 + B * (U + 1) * (H + 1)], dtype=torch.float32, device=cuda)

  def call():
    nat._check(nat.lib().lt_joint_string_rows(
        ctypes.byref(graph.g), ctypes.byref(pb), ctypes.byref(jp), nat._ptr(nf), nat._ptr(lab),
        nat._ptr(nl), nat._ptr(Ws), nat._ptr(states), nat._ptr(ws), ws.numel() * 4,
        nat._stream()), 'lt_joint_string_rows')

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
    want = nat.joint_string_rows(graph, pc, pf, wo, bias, nf, lab, nl, precision, dtype)
    for got, w in zip((Ws, states), want):
      assert torch.equal(_bits(got), _bits(w))
