"""Prefix beam search on the GPU (RecognitionLattice.beam_search ->
lt_table_beam_search, lt_beam.hip).

* MaxTropical, bit for bit: the scores are fp32 adds and maxes in a fixed
  order, so labels, num_labels, scores, trace and step_score equal
  cpu.beam_search's on the same fp32 weights. The shapes cover the LDS ring
  (with a T and num_frames that are no multiple of it), a full wave of slots,
  the greedy beam, bf16 weights, rows longer than a wave and the path without
  a ring.
* Log: beam_ref.replay judges every frame of the kernel's trace / step_score
  on its own, in float64 with merges by prefix identity; the final outputs
  must be the last live frame's slots and the NumPy backtrace of the trace.
* The exhaustive V = 2 lattice, degenerate inputs, the C ABI's error codes,
  the restatement past K = 64, reruns, poisoned and stale buffers, and a
  captured graph replayed on new weights.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import last_torch_amd as lt
from last_torch_amd import _native as nat
from last_torch_amd import cpu
from poisoned_buffers import poisoned, stale
import beam_ref as ref
import sample_ref

pytestmark = pytest.mark.gpu

SEMIRINGS = {'Log': lt.semirings.Log, 'MaxTropical': lt.semirings.MaxTropical}
SID = {'Log': nat.SEMIRING_LOG, 'MaxTropical': nat.SEMIRING_MAX}

_bigram32 = lambda rng: lt.contexts.FullNGram(vocab_size=32, context_size=1)
# name: (context factory, K, T, dtype, blank bias)
CASES = {
    # a frame of 4.4 KB: a ring of 7 frames; T = 70 and nf = 67 are no multiples
    'bigram_v32_k16': (_bigram32, 16, 70, torch.float32, 3.0),
    'bigram_v32_k64': (_bigram32, 64, 24, torch.float32, 3.0),     # a full wave of slots
    'bigram_v32_k1': (_bigram32, 1, 40, torch.float32, 3.0),       # greedy
    'bigram_v32_bf16': (_bigram32, 16, 40, torch.bfloat16, 3.0),
    'trigram_v5': (lambda rng: lt.contexts.FullNGram(vocab_size=5, context_size=2), 8, 30,
                   torch.float32, 1.5),
    'table_c17_v6': (lambda rng: lt.contexts.NextStateTable(sample_ref.random_table(rng, 17, 6)),
                     8, 30, torch.float32, 1.5),
    # a row longer than a wave, a label mask of four words
    'table_c5_v100': (lambda rng: lt.contexts.NextStateTable(sample_ref.random_table(rng, 5, 100)),
                      16, 12, torch.float32, 3.0),
    # a frame of 35 KB: no ring, and a table too large for LDS
    'table_c300_v28': (lambda rng: lt.contexts.NextStateTable(
        sample_ref.random_table(rng, 300, 28)), 8, 20, torch.float32, 3.0),
}


@functools.lru_cache(maxsize=None)
def _case(name):
  """(context, table, K, nf, W fp32 as the kernel sees it, dtype): built once."""
  make, K, T, dtype, bias = CASES[name]
  rng = np.random.default_rng(sum(map(ord, name)))
  context = make(rng)
  table = sample_ref.table_of(context)
  C, V = table.shape
  nf = [T, T - 3, 1, 0]
  W = torch.tensor(ref.make_weights(rng, 4, T, C, V, bias)).to(dtype).float().numpy()
  return context, table, K, nf, W, dtype


@functools.lru_cache(maxsize=None)
def _host(name, semiring):
  """cpu.beam_search on the host, with its trace, as numpy: computed once."""
  context, _, K, nf, W, _ = _case(name)
  out = cpu.beam_search(torch.tensor(W), torch.tensor(nf), context, K, SEMIRINGS[semiring],
                        want_trace=True)
  return tuple(x.numpy() for x in out)


def _kernel(context, W, nf, K, semiring, device, dtype=torch.float32, want_trace=True):
  """lt_table_beam_search through the binding, as numpy."""
  graph = nat.TableGraph(sample_ref.table_of(context), 0, device)
  Wd = torch.as_tensor(W).to(device=device, dtype=dtype).contiguous()
  nfd = torch.tensor(nf, dtype=torch.int32, device=device)
  assert nat.table_beam_search_supported(graph, Wd, K)
  out = nat.table_beam_search(graph, Wd, nfd, K, SID[semiring], want_trace=want_trace)
  torch.cuda.synchronize()
  return tuple(x.cpu().numpy() for x in out)


@pytest.mark.parametrize('name', list(CASES))
def test_max_tropical_bit_exact(cuda, name):
  context, _, K, nf, W, dtype = _case(name)
  got = _kernel(context, W, nf, K, 'MaxTropical', cuda, dtype)
  want = _host(name, 'MaxTropical')
  for g, w, what in zip(got, want, ('labels', 'num_labels', 'scores', 'trace', 'step_score')):
    assert g.shape == w.shape, what
    assert np.array_equal(g, w), (what, np.argwhere(g != w)[:4])
  assert got[1].dtype == np.int32 and got[0].dtype == np.int64 and got[3].dtype == np.int32


@pytest.mark.parametrize('name', list(CASES))
def test_log_replay(cuda, name):
  context, table, K, nf, W, dtype = _case(name)
  labels, nl, scores, trace, step = _kernel(context, W, nf, K, 'Log', cuda, dtype)
  steps, final = ref.replay(W, nf, table, K, 'Log', trace, step)
  assert steps == sum(nf)
  ref.check_outputs(final, trace, nf, labels, nl, scores)
  if K > 1:
    assert len(final[0]) == K   # the beam filled: candidates were pruned
  # merging matters on these inputs: the summed score is not the best alignment's
  if K > 1:
    assert abs(scores[0, 0] - _host(name, 'MaxTropical')[2][0, 0]) > 1e-2
  # without the trace outputs (backpointers in the workspace): the same beams
  again = _kernel(context, W, nf, K, 'Log', cuda, dtype, want_trace=False)
  assert len(again) == 3
  for g, w in zip(again, (labels, nl, scores)):
    assert np.array_equal(g, w)


def _lattice(context, table, K=0):
  align = lt.alignments.FrameDependent() if K == 0 else lt.alignments.FrameLabelDependent(K)
  return lt.RecognitionLattice(
      context=context, alignment=align,
      weight_fn_cacher_factory=lambda _: lt.weight_fns.NullCacher(),
      weight_fn_factory=lambda _: lt.weight_fns.TableWeightFn(table))


def _frames(B, T, device):
  return torch.arange(T, dtype=torch.float32, device=device)[None, :, None].expand(B, T, 1)


def _api(context, W, nf, K, semiring, device):
  B, T = W.shape[:2]
  lat = _lattice(context, torch.as_tensor(W).to(device))
  out = lat.beam_search(_frames(B, T, device), torch.tensor(nf, device=device), K,
                        SEMIRINGS[semiring])
  labels, nl, scores = out
  assert labels.is_cuda and labels.dtype == torch.int64 and tuple(labels.shape) == (B, K, T)
  assert nl.dtype == torch.int64 and scores.dtype == torch.float32
  return lat, labels, nl, scores


def test_exhaustive_v2_t5(cuda):
  rng = np.random.default_rng(11)
  V, T, K = 2, 5, 64
  context = lt.contexts.FullNGram(vocab_size=V, context_size=1)
  W = ref.make_weights(rng, 1, T, V + 1, V, 1.5)
  lat, labels, nl, scores = _api(context, W, [T], K, 'Log', cuda)
  live = scores[0] > -np.inf
  assert int(live.sum()) == 63 and bool(live[:63].all())
  seqs = {tuple(labels[0, r, :nl[0, r]].tolist()) for r in range(63)}
  assert len(seqs) == 63 and all(0 not in s for s in seqs)
  lat_k = _lattice(context, torch.tensor(W).to(cuda).repeat_interleave(K, dim=0))
  nfk = torch.full([K], T, device=cuda)
  want = lat_k._string_forward(None, _frames(K, T, cuda), nfk, labels[0], nl[0], lt.semirings.Log)
  np.testing.assert_allclose(scores[0, :63].cpu().numpy(), want[:63].cpu().numpy(), rtol=0,
                             atol=1e-4)
  log_z, _ = lat._forward(None, _frames(1, T, cuda), torch.tensor([T], device=cuda),
                          lt.semirings.Log)
  assert abs(float(torch.logsumexp(scores[0, :63], 0)) - float(log_z[0])) <= 1e-4
  _, mlab, mnl, mscores = _api(context, W, [T], K, 'MaxTropical', cuda)
  path, _, weight = lat.shortest_path(_frames(1, T, cuda), torch.tensor([T], device=cuda),
                                      label_convention='true')
  assert abs(float(mscores[0, 0]) - float(weight[0])) <= 1e-4
  assert mlab[0, 0, :mnl[0, 0]].tolist() == [y for y in path[0].tolist() if y]


def test_dead_beams_masked_arcs_and_empty_utterances(cuda):
  rng = np.random.default_rng(5)
  context = lt.contexts.FullNGram(vocab_size=3, context_size=1)
  table = sample_ref.table_of(context)
  B, T, K = 4, 8, 6
  W = ref.make_weights(rng, B, T, 4, 3, 1.5)
  W[1] = -np.inf                        # no arc at all: an all-dead beam
  W[2, :, :, 2] = -np.inf               # label 2 masked everywhere
  W[2, 3, :, 0] = -np.inf               # and no blank on frame 3
  nf = [T, T, T, 0]
  for semiring in SEMIRINGS:
    labels, nl, scores, trace, step = _kernel(context, W, nf, K, semiring, cuda)
    steps, final = ref.replay(W, nf, table, K, semiring, trace, step)
    assert steps == 3 * T
    ref.check_outputs(final, trace, nf, labels, nl, scores)
    assert (scores[1] == -np.inf).all() and not labels[1].any() and not nl[1].any()
    assert np.isfinite(scores[[0, 2]]).all() and (labels[2] != 2).all()
    assert scores[3, 0] == 0 and (scores[3, 1:] == -np.inf).all() and not labels[3].any()
  want = cpu.beam_search(torch.tensor(W), torch.tensor(nf), context, K, lt.semirings.MaxTropical)
  for g, w in zip((labels, nl, scores), want):
    assert np.array_equal(g, w.numpy())


def test_abi_error_codes(cuda):
  """LT_EINVAL for beam_size = 0, the Real semiring, a NULL output and a NULL
  trace without a workspace; LT_EUNSUPPORTED for expansions >= 1 and K = 65;
  nothing is launched, so the outputs stay untouched."""
  lib = nat.lib()
  V, T, B, K = 4, 6, 2, 3
  context = lt.contexts.FullNGram(vocab_size=V, context_size=1)
  W = torch.randn([B, T, V + 1, V + 1], device=cuda)
  nf = torch.tensor([T, 4], dtype=torch.int32, device=cuda)
  graph = nat.TableGraph(context.next_state_table(), 0, cuda)
  fld = nat.TableGraph(context.next_state_table(), 1, cuda)
  labels = torch.full([B, 65, T], -7, dtype=torch.int64, device=cuda)
  nl = torch.full([B, 65], -7, dtype=torch.int32, device=cuda)
  scores = torch.full([B, 65], -7.0, device=cuda)
  trace = torch.full([B, T, 65], -7, dtype=torch.int32, device=cuda)
  step = torch.full([B, T, 65], -7.0, device=cuda)
  pb = nat.TableProblem(B, T, 0, nat.LT_DTYPE_F32)
  stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

  def call(g, beam, sid=nat.SEMIRING_LOG, lab=labels, tr=trace, ws=None, nbytes=0):
    return lib.lt_table_beam_search(ctypes.byref(g.g), ctypes.byref(pb), ptr(W), ptr(nf), beam,
                                    sid, ptr(lab), ptr(nl), ptr(scores), ptr(tr), ptr(step),
                                    ptr(ws), nbytes, stream)

  def query(g, beam):
    nbytes = ctypes.c_size_t(99)
    rc = lib.lt_table_beam_search_workspace_bytes(ctypes.byref(g.g), ctypes.byref(pb), beam,
                                                  ctypes.byref(nbytes))
    return rc, nbytes.value

  assert call(graph, 0) == -1 and query(graph, 0)[0] == -1
  assert call(fld, K) == nat.LT_EUNSUPPORTED and query(fld, K)[0] == nat.LT_EUNSUPPORTED
  assert call(graph, 65) == nat.LT_EUNSUPPORTED and query(graph, 65)[0] == nat.LT_EUNSUPPORTED
  assert call(graph, K, sid=nat.SEMIRING_REAL) == -1
  assert call(graph, K, lab=None) == -1
  assert call(graph, K, tr=None) == -1                      # no trace and no workspace
  assert query(graph, K) == (0, 4 * B * T * K)
  small = torch.empty([4 * B * T * K - 4], dtype=torch.uint8, device=cuda)
  assert call(graph, K, tr=None, ws=small, nbytes=small.numel()) == -1
  torch.cuda.synchronize()
  for t in (labels, nl, trace):
    assert (t == -7).all()
  assert (scores == -7).all() and (step == -7).all()          # nothing was launched
  assert not nat.table_beam_search_supported(graph, W, 65)
  assert not nat.table_beam_search_supported(fld, W, K)


def test_k65_runs_the_restatement_on_the_device(cuda):
  rng = np.random.default_rng(65)
  context = lt.contexts.FullNGram(vocab_size=5, context_size=1)
  nf = [12, 9, 1, 0]
  W = ref.make_weights(rng, 4, 12, 6, 5, 1.5)
  _, labels, nl, scores = _api(context, W, nf, 65, 'MaxTropical', cuda)
  want = cpu.beam_search(torch.tensor(W), torch.tensor(nf), context, 65, lt.semirings.MaxTropical)
  assert int((scores[0] > -np.inf).sum()) == 65
  for g, w in zip((labels, nl, scores), want):
    assert torch.equal(g.cpu(), w)
  # Log: the device's logaddexp may round differently from the host's
  _, _, _, lscores = _api(context, W, nf, 65, 'Log', cuda)
  lwant = cpu.beam_search(torch.tensor(W), torch.tensor(nf), context, 65, lt.semirings.Log)[2]
  fin = torch.isfinite(lwant)
  assert torch.equal(torch.isfinite(lscores.cpu()), fin)
  np.testing.assert_allclose(lscores.cpu()[fin].numpy(), lwant[fin].numpy(), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize('mode', ['poisoned', 'stale'])
@pytest.mark.parametrize('want_trace', [True, False])
def test_poisoned_and_stale_buffers(cuda, mode, want_trace):
  """Every output element and every workspace byte read is written by the
  call: on 0xFF-filled buffers, and on the buffers a finished call on other
  weights left, the bits are those of a plain run -- which reruns bit-equal."""
  context, _, K, nf, W, _ = _case('bigram_v32_k16')
  graph = nat.TableGraph(sample_ref.table_of(context), 0, cuda)
  nfd = torch.tensor(nf, dtype=torch.int32, device=cuda)
  Wb = torch.tensor(W, device=cuda)
  Wa = torch.tensor(W[::-1].copy(), device=cuda)
  nfa = torch.tensor(nf[::-1], dtype=torch.int32, device=cuda)
  fn = lambda x: nat.table_beam_search(graph, x[0], x[1], K, nat.SEMIRING_LOG,
                                       want_trace=want_trace)
  plain = [t.clone() for t in fn((Wb, nfd))]
  rerun = fn((Wb, nfd))
  torch.cuda.synchronize()
  for p, r in zip(plain, rerun):
    assert torch.equal(p, r)
  if mode == 'poisoned':
    with poisoned(nat):
      out = fn((Wb, nfd))
  else:
    with stale(nat) as s:
      s.record(fn, (Wa, nfa))
      torch.cuda.synchronize()
      out = s.replay(fn, (Wb, nfd))
  torch.cuda.synchronize()
  assert len(out) == len(plain) == (5 if want_trace else 3)
  for p, o in zip(plain, out):
    assert torch.equal(p.view(torch.uint8), o.view(torch.uint8))


def test_graph_replays_match_eager(cuda):
  """lt_table_beam_search captured on one stream (a single kernel: no memset,
  no second launch) and replayed on new weights equals eager calls."""
  context, _, K, nf, W, _ = _case('bigram_v32_k16')
  B, T = W.shape[:2]
  graph = nat.TableGraph(sample_ref.table_of(context), 0, cuda)
  nfd = torch.tensor(nf, dtype=torch.int32, device=cuda)
  Wd = torch.tensor(W, device=cuda)
  pb = nat._tproblem(graph, Wd)
  labels = torch.empty([B, K, T], dtype=torch.int64, device=cuda)
  nl = torch.empty([B, K], dtype=torch.int32, device=cuda)
  scores = torch.empty([B, K], device=cuda)
  ws = torch.empty([4 * B * T * K], dtype=torch.uint8, device=cuda)

  def call():
    nat._check(nat.lib().lt_table_beam_search(
        ctypes.byref(graph.g), ctypes.byref(pb), nat._ptr(Wd), nat._ptr(nfd), K,
        nat.SEMIRING_LOG, nat._ptr(labels), nat._ptr(nl), nat._ptr(scores), None, None,
        nat._ptr(ws), ws.numel(), nat._stream()), 'lt_table_beam_search')

  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(s):
    call()  # eager on the side stream first, as torch's capture recipe does
  torch.cuda.current_stream().wait_stream(s)
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    call()
  first = None
  for seed in (2, 3):
    W2 = torch.tensor(ref.make_weights(np.random.default_rng(seed), B, T, 33, 32, 3.0),
                      device=cuda)
    Wd.copy_(W2)
    g.replay()
    torch.cuda.synchronize()
    el, en, es = nat.table_beam_search(graph, W2, nfd, K, nat.SEMIRING_LOG)
    torch.cuda.synchronize()
    assert torch.equal(labels, el) and torch.equal(nl, en) and torch.equal(scores, es)
    if first is None:
      first = es.clone()
  assert not torch.equal(first, scores)   # the replays did see the new weights
