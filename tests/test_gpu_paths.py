"""Path scoring and the path scatter on the GPU (lt_table_path_score /
lt_table_path_scatter, lt_paths.hip) against the NumPy restatement path_ref.

* Score: the labels the GPU's own lt_table_sample drew score to its
  path_weight bit for bit, and the states equal the reference walk exactly (-1
  on padding frames), on shapes that cover bf16, the 64-frame label loads'
  boundaries (num_frames 130, 129, 128, 65, 64, 1, 0), a second workgroup per
  utterance, the table staged in LDS and read from memory (the V = 32 trigram's
  135 KB), and a table whose labels loop on their state. Given (not sampled)
  labels: invalid ones give -inf and states -1, labels on padding frames are
  ignored.
* Scatter: an integer-valued grad equals the float64 reference exactly, a
  random one within S 2^-24 sum_s |g_s| per element (the fp32 bound of an
  S-term sum); paths forced to share arcs (one path three times; nine samples
  of peaked weights); every element off the paths is exactly 0.0; two runs are
  bit-equal.
* Every output of the three wrappers on poisoned and stale allocations.
* One HIP-graph capture of score + scatter + distance on a single stream,
  replayed on new inputs, against the eager results.
"""
import numpy as np
import pytest
import torch

import last_torch_amd as lt
from last_torch_amd import _native as nat
from poisoned_buffers import poisoned, stale
import path_ref
import sample_ref

pytestmark = pytest.mark.gpu


def _self_loops(rng, C, V):
  """A random table in which half of the labels keep the state."""
  tab = rng.integers(0, C, [C, V]).astype(np.int32)
  keep = rng.random([C, V]) < 0.5
  tab[keep] = np.broadcast_to(np.arange(C, dtype=np.int32)[:, None], [C, V])[keep]
  return torch.tensor(tab)


RAGGED = [130, 129, 128, 65, 64, 1, 0]
# name: (context factory, T, num_frames, S, dtype)
CASES = {
    'bigram_v32': (lambda rng: lt.contexts.FullNGram(vocab_size=32, context_size=1), 70,
                   [70, 67, 1, 0], 5, torch.float32),
    'bigram_v32_bf16': (lambda rng: lt.contexts.FullNGram(vocab_size=32, context_size=1), 70,
                        [70, 67, 1, 0], 5, torch.bfloat16),
    # every boundary of the 64-frame loads; 9 paths: two workgroups an utterance
    'bigram_v32_t130': (lambda rng: lt.contexts.FullNGram(vocab_size=32, context_size=1), 130,
                        RAGGED, 9, torch.float32),
    'trigram_v5': (lambda rng: lt.contexts.FullNGram(vocab_size=5, context_size=2), 70,
                   [70, 67, 1, 0], 5, torch.float32),
    # a 33 KB table, staged
    'table_c300_v28': (lambda rng: lt.contexts.NextStateTable(sample_ref.random_table(rng, 300, 28)),
                       70, [70, 67, 1, 0], 5, torch.float32),
    # a 135 KB table: read from memory
    'trigram_v32': (lambda rng: lt.contexts.FullNGram(vocab_size=32, context_size=2), 6, [6, 4], 5,
                    torch.float32),
    'table_self_loops': (lambda rng: lt.contexts.NextStateTable(_self_loops(rng, 17, 6)), 70,
                         [70, 67, 1, 0], 5, torch.float32),
}
_CACHE = {}


def _case(name, cuda):
  """The problem, the GPU's own samples and the reference's score of them,
  computed once and shared (read-only)."""
  if name not in _CACHE:
    make, T, nf, S, dtype = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    context = make(rng)
    table = sample_ref.table_of(context)
    C, V = table.shape
    B = len(nf)
    Wd = torch.tensor(rng.standard_normal([B, T, C, V + 1]).astype(np.float32)).to(cuda, dtype)
    W = Wd.float().cpu().numpy()  # bf16 weights are widened exactly
    nfd = torch.tensor(nf, dtype=torch.int32, device=cuda)
    graph = nat.TableGraph(table, 0, cuda)
    log_z, alpha = nat.table_forward(graph, Wd, nfd, nat.SEMIRING_LOG)
    labels, weights = nat.table_sample(graph, Wd, nfd, log_z, alpha, S, 0xfeed + len(name))
    ref = path_ref.score(W, nf, table, labels.cpu().numpy())
    for x in (W,) + ref:
      x.setflags(write=False)
    _CACHE[name] = dict(table=table, graph=graph, Wd=Wd, W=W, nf=nf, nfd=nfd, labels=labels,
                        weights=weights, ref=ref, context=context)
  return _CACHE[name]


@pytest.mark.parametrize('name', list(CASES))
def test_sampled_labels_score_bit_for_bit(cuda, name):
  c = _case(name, cuda)
  got, states = nat.table_path_score(c['graph'], c['Wd'], c['nfd'], c['labels'])
  w32, _, _, want_states = c['ref']
  assert got.dtype == torch.float32 and states.dtype == torch.int32
  assert torch.equal(got, c['weights'])                       # lt_table_sample's own sums
  np.testing.assert_array_equal(got.cpu().numpy(), w32)
  np.testing.assert_array_equal(states.cpu().numpy(), want_states)
  assert np.isfinite(w32).all()
  only, none = nat.table_path_score(c['graph'], c['Wd'], c['nfd'], c['labels'], want_states=False)
  assert none is None and torch.equal(only, got)


@pytest.mark.parametrize('name', ['bigram_v32_t130', 'trigram_v32', 'table_self_loops'])
def test_given_labels_invalid_and_padding(cuda, name):
  c = _case(name, cuda)
  rng = np.random.default_rng(5)
  table, nf = c['table'], c['nf']
  V = table.shape[1]
  B, S, T = c['labels'].shape
  labels = rng.integers(0, V + 1, [B, S, T])
  labels[rng.random([B, S, T]) < 0.5] = 0
  for b in range(B):                                          # junk on the padding frames
    labels[b, :, nf[b]:] = rng.integers(-5, V + 9, [S, T - nf[b]])
  labels[0, 1, nf[0] - 1] = V + 1                             # the last live frame
  labels[0, 2, 0] = -1
  labels[1, 0, nf[1] // 2] = 1 << 40                          # past int32
  got, states = nat.table_path_score(c['graph'], c['Wd'], c['nfd'],
                                     torch.tensor(labels, device=cuda))
  w32, _, _, want_states = path_ref.score(c['W'], nf, table, labels)
  got = got.cpu().numpy()
  assert not np.isnan(got).any()
  assert got[0, 1] == -np.inf and got[0, 2] == -np.inf and got[1, 0] == -np.inf
  np.testing.assert_array_equal(got, w32)
  np.testing.assert_array_equal(states.cpu().numpy(), want_states)


def _scatter_check(c, labels, states, grad, exact):
  dW = nat.table_path_scatter(c['graph'], c['Wd'], c['nfd'], labels, states,
                              torch.tensor(grad, device=labels.device))
  again = nat.table_path_scatter(c['graph'], c['Wd'], c['nfd'], labels, states,
                                 torch.tensor(grad, device=labels.device))
  assert dW.dtype == torch.float32 and tuple(dW.shape) == tuple(c['Wd'].shape)
  assert torch.equal(dW, again)
  got = dW.cpu().numpy()
  want, mag = path_ref.scatter(c['W'].shape, c['nf'], labels.cpu().numpy(), states.cpu().numpy(),
                               grad)
  if exact:
    np.testing.assert_array_equal(got, want)
  else:
    assert (np.abs(got - want) <= labels.shape[1] * 2.0**-24 * mag).all()
  off = mag == 0
  assert off.any() and not got[off].any() and not np.signbit(got[off]).any()  # exactly +0.0
  return got


@pytest.mark.parametrize('name', list(CASES))
def test_scatter_against_the_reference(cuda, name):
  c = _case(name, cuda)
  rng = np.random.default_rng(9)
  labels = c['labels']
  states = torch.tensor(c['ref'][3], device=cuda)
  B, S, _ = labels.shape
  _scatter_check(c, labels, states, rng.integers(-4, 5, [B, S]).astype(np.float32), True)
  _scatter_check(c, labels, states, rng.standard_normal([B, S]).astype(np.float32), False)


def test_scatter_forced_collisions(cuda):
  c = _case('bigram_v32', cuda)
  rng = np.random.default_rng(10)
  # the same path three times among five
  labels = c['labels'].clone()
  labels[:, 2] = labels[:, 0]
  labels[:, 4] = labels[:, 0]
  _, states = nat.table_path_score(c['graph'], c['Wd'], c['nfd'], labels)
  B, S, _ = labels.shape
  got = _scatter_check(c, labels, states, np.full([B, S], 1.0, np.float32), True)
  assert got.max() >= 3.0
  _scatter_check(c, labels, states, rng.standard_normal([B, S]).astype(np.float32), False)
  # nine samples of peaked weights: one arc per state dominates, so samples share arcs
  table = c['table']
  C, V = table.shape
  T, S = 70, 9
  W = rng.standard_normal([4, T, C, V + 1]).astype(np.float32)
  peak = rng.integers(0, V + 1, [4, T, C])
  np.put_along_axis(W, peak[..., None], 12.0, axis=-1)
  Wd = torch.tensor(W, device=cuda)
  log_z, alpha = nat.table_forward(c['graph'], Wd, c['nfd'], nat.SEMIRING_LOG)
  labels, _ = nat.table_sample(c['graph'], Wd, c['nfd'], log_z, alpha, S, 77)
  _, states = nat.table_path_score(c['graph'], Wd, c['nfd'], labels)
  peaked = dict(c, Wd=Wd, W=W)
  got = _scatter_check(peaked, labels, states, np.ones([4, S], np.float32), True)
  assert got.max() >= 5.0                                      # most samples share the peak arcs
  _scatter_check(peaked, labels, states, rng.standard_normal([4, S]).astype(np.float32), False)


def _edit_inputs(rng, B, S, T, U, cuda):
  hyp = torch.tensor(rng.integers(0, 4, [B, S, T]), device=cuda)
  ref = torch.tensor(rng.integers(0, 4, [B, U]).astype(np.int32), device=cuda)
  nl = torch.tensor(rng.integers(0, U + 1, [B]).astype(np.int32), device=cuda)
  return hyp, ref, nl


@pytest.mark.parametrize('mode', ['poisoned', 'stale'])
def test_outputs_on_poisoned_and_stale_allocations(cuda, mode):
  """Every element of every output is written: on allocations full of 0xFF
  bytes, and on the allocations a finished call on another problem left."""
  c = _case('bigram_v32', cuda)
  rng = np.random.default_rng(11)
  B, S, T = c['labels'].shape
  U = 20
  other = nat.table_sample(c['graph'], c['Wd'], torch.flip(c['nfd'], [0]),
                           *nat.table_forward(c['graph'], c['Wd'], torch.flip(c['nfd'], [0]),
                                              nat.SEMIRING_LOG), S, 3)[0]
  grads = [torch.tensor(rng.standard_normal([B, S]).astype(np.float32), device=cuda)
           for _ in range(2)]
  edits = [_edit_inputs(rng, B, S, T, U, cuda) for _ in range(2)]

  def fn(p):
    nfd, labels, grad, (hyp, ref, nl) = p
    weight, states = nat.table_path_score(c['graph'], c['Wd'], nfd, labels)
    dW = nat.table_path_scatter(c['graph'], c['Wd'], nfd, labels, states, grad)
    dist, length = nat.edit_distance(hyp, nfd, ref, nl)
    return weight, states, dW, dist, length

  a = (torch.flip(c['nfd'], [0]), other, grads[0], edits[0])
  b = (c['nfd'], c['labels'], grads[1], edits[1])
  if mode == 'poisoned':
    with poisoned(nat):
      out = fn(b)
  else:
    with stale(nat) as s:
      s.record(fn, a)
      torch.cuda.synchronize()
      out = s.replay(fn, b)
  torch.cuda.synchronize()
  weight, states, dW, dist, length = (x.cpu().numpy() for x in out)
  w32, _, _, want_states = c['ref']
  np.testing.assert_array_equal(weight, w32)
  np.testing.assert_array_equal(states, want_states)
  want, mag = path_ref.scatter(c['W'].shape, c['nf'], c['labels'].cpu().numpy(), want_states,
                               grads[1].cpu().numpy())
  assert (np.abs(dW - want) <= S * 2.0**-24 * mag).all() and not dW[mag == 0].any()
  hyp, ref, nl = (x.cpu().numpy() for x in edits[1])
  wd, wl = path_ref.edit_distance(hyp, c['nf'], ref, nl)
  np.testing.assert_array_equal(dist, wd)
  np.testing.assert_array_equal(length, wl)


def test_graph_capture_and_replay(cuda):
  """score + scatter + distance captured on one stream; the replay on new
  inputs gives the eager call's bits."""
  import ctypes
  c = _case('bigram_v32', cuda)
  rng = np.random.default_rng(12)
  graph = c['graph']
  B, S, T = c['labels'].shape
  U = 20
  W = c['Wd'].clone()
  labels = c['labels'].clone()
  nfd = c['nfd']
  grad = torch.ones([B, S], device=cuda)
  hyp, ref, nl = _edit_inputs(rng, B, S, T, U, cuda)
  weight = torch.empty([B, S], device=cuda)
  states = torch.empty([B, S, T], dtype=torch.int32, device=cuda)
  dW = torch.empty(tuple(W.shape), device=cuda)
  dist = torch.empty([B, S], dtype=torch.int32, device=cuda)
  length = torch.empty([B, S], dtype=torch.int32, device=cuda)
  pb = nat._tproblem(graph, W)
  lib = nat.lib()

  def call():
    st = nat._stream()
    nat._check(lib.lt_table_path_score(ctypes.byref(graph.g), ctypes.byref(pb), nat._ptr(W),
                                       nat._ptr(nfd), nat._ptr(labels), S, nat._ptr(weight),
                                       nat._ptr(states), st), 'lt_table_path_score')
    nat._check(lib.lt_table_path_scatter(ctypes.byref(graph.g), ctypes.byref(pb), nat._ptr(nfd),
                                         nat._ptr(labels), nat._ptr(states), S, nat._ptr(grad),
                                         nat._ptr(dW), st), 'lt_table_path_scatter')
    nat._check(lib.lt_edit_distance(B, S, T, U, nat._ptr(hyp), nat._ptr(nfd), nat._ptr(ref),
                                    nat._ptr(nl), nat._ptr(dist), nat._ptr(length), st),
               'lt_edit_distance')

  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(s):
    call()  # eager on the side stream first, as torch's capture recipe does
  torch.cuda.current_stream().wait_stream(s)
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    call()
  first = weight.clone()
  for seed in (2, 3):
    r = np.random.default_rng(seed)
    W.copy_(torch.tensor(r.standard_normal(tuple(W.shape)).astype(np.float32), device=cuda))
    V = graph.V
    labels.copy_(torch.tensor(r.integers(0, V + 1, [B, S, T]), device=cuda))
    grad.copy_(torch.tensor(r.standard_normal([B, S]).astype(np.float32), device=cuda))
    hyp.copy_(torch.tensor(r.integers(0, 4, [B, S, T]), device=cuda))
    g.replay()
    torch.cuda.synchronize()
    ew, es = nat.table_path_score(graph, W, nfd, labels)
    edW = nat.table_path_scatter(graph, W, nfd, labels, es, grad)
    ed, el = nat.edit_distance(hyp, nfd, ref, nl)
    torch.cuda.synchronize()
    assert torch.equal(weight, ew) and torch.equal(states, es) and torch.equal(dW, edW)
    assert torch.equal(dist, ed) and torch.equal(length, el)
    np.testing.assert_array_equal(
        ed.cpu().numpy(),
        path_ref.edit_distance(hyp.cpu().numpy(), c['nf'], ref.cpu().numpy(),
                               nl.cpu().numpy())[0])
  assert not torch.equal(weight, first)  # the replays did see the new inputs
