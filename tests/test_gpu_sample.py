"""Path sampling on the GPU (RecognitionLattice.sample -> lt_den_forward /
lt_table_forward + lt_table_sample, lt_sample.hip).

* Step replay: every step of every sampled path is recomputed in float64 from
  a float64 alpha and the specified noise (NumPy Philox, sample_ref); the
  kernel's pick must score at least best - 2 (1e-4 + 1e-4 |best|), the
  project's alpha parity bound once for each of the two scores compared. A
  wrong noise word, candidate set or tie order fails almost every step, since
  the gaps between Gumbel-perturbed scores are O(1). The shapes cover the LDS
  ring at several depths (and a T and num_frames that are no multiple of it),
  the staged and the unstaged in-arc CSR, states of more than 64 in-arcs, the
  path without a ring, bf16 weights and a second workgroup per utterance.
* Distribution: the 81 paths of test_sample_cpu's bigram, and every arc's
  count against S times the oracle's Log marginal, both within
  5 (sqrt(S p (1 - p)) + 1).
* Validity, the weight's fp32 summation bound, determinism, the S-prefix
  property, unsampled and empty utterances, and the C ABI's error codes.
"""
import ctypes

import numpy as np
import pytest
import torch

import last_torch_amd as lt
from last_torch_amd import _native as nat
import sample_ref as ref

pytestmark = pytest.mark.gpu


def _lattice(context, table, K=0):
  align = lt.alignments.FrameDependent() if K == 0 else lt.alignments.FrameLabelDependent(K)
  return lt.RecognitionLattice(
      context=context, alignment=align,
      weight_fn_cacher_factory=lambda _: lt.weight_fns.NullCacher(),
      weight_fn_factory=lambda _: lt.weight_fns.TableWeightFn(table))


def _sample(context, W, nf, S, seed, device, dtype=torch.float32):
  """RecognitionLattice.sample on ROCm tensors, as numpy."""
  B, T = W.shape[:2]
  lat = _lattice(context, torch.as_tensor(W).to(device=device, dtype=dtype))
  frames = torch.arange(T, dtype=torch.float32, device=device)[None, :, None].expand(B, T, 1)
  labels, weights, log_z = lat.sample(frames, torch.tensor(nf, device=device), S, seed)
  assert labels.is_cuda and labels.dtype == torch.int64 and tuple(labels.shape) == (B, S, T)
  assert weights.dtype == torch.float32 and tuple(weights.shape) == (B, S)
  assert tuple(log_z.shape) == (B,)
  return labels.cpu().numpy(), weights.cpu().numpy(), log_z.cpu().numpy()


def _two_sinks(C, V):
  """Every arc leads to state 1 or 2: in-degrees C*V/2 > 64."""
  return torch.tensor((1 + (np.arange(C * V) % 2)).reshape(C, V).astype(np.int32))


# name: (context factory, T, B, S, dtype)
REPLAYS = {
    # 34 candidates a step; 5 waves -> a ring of 4 frames, T = 70 and nf = 67 no multiple
    'bigram_v32': (lambda rng: lt.contexts.FullNGram(vocab_size=32, context_size=1), 70, 4, 5,
                   torch.float32),
    'bigram_v32_bf16': (lambda rng: lt.contexts.FullNGram(vocab_size=32, context_size=1), 70, 4,
                        5, torch.bfloat16),
    # 9 samples: two workgroups an utterance, the second with one sampling
    # wave; 8 waves -> a ring of 7 frames, T = 71 no multiple
    'bigram_v32_two_groups': (lambda rng: lt.contexts.FullNGram(vocab_size=32, context_size=1),
                              71, 4, 9, torch.float32),
    'trigram_v5': (lambda rng: lt.contexts.FullNGram(vocab_size=5, context_size=2), 30, 4, 5,
                   torch.float32),
    'table_c17_v6': (lambda rng: lt.contexts.NextStateTable(ref.random_table(rng, 17, 6)), 30, 4,
                     5, torch.float32),
    # in-degree 120: the sliced reduction with a running best
    'table_c40_v6_two_sinks': (lambda rng: lt.contexts.NextStateTable(_two_sinks(40, 6)), 12, 4,
                               5, torch.float32),
    # a frame of 35 KB: no ring, and a CSR too large for LDS
    'table_c300_v28': (lambda rng: lt.contexts.NextStateTable(ref.random_table(rng, 300, 28)),
                       20, 4, 5, torch.float32),
    # a ring of one frame with the CSR left in memory
    'table_c220_v30_ring': (lambda rng: lt.contexts.NextStateTable(ref.random_table(rng, 220, 30)),
                            8, 4, 8, torch.float32),
    # 139 KB a frame: the no-ring path
    'trigram_v32': (lambda rng: lt.contexts.FullNGram(vocab_size=32, context_size=2), 6, 2, 5,
                    torch.float32),
}


@pytest.mark.parametrize('name', list(REPLAYS))
def test_step_replay(cuda, name):
  make, T, B, S, dtype = REPLAYS[name]
  rng = np.random.default_rng(sum(map(ord, name)))
  context = make(rng)
  table = ref.table_of(context)
  C, V = table.shape
  nf = [T, T - 3, 1, 0][:B]
  W = torch.tensor(rng.standard_normal([B, T, C, V + 1]).astype(np.float32)).to(dtype)
  W = W.float().numpy()  # bf16 weights are widened exactly
  seed = 0x5eed0000cafe + len(name)
  labels, weights, log_z = _sample(context, W, nf, S, seed, cuda, dtype)
  want_z, alpha = ref.forward(W, nf, table)
  np.testing.assert_allclose(log_z, want_z, rtol=1e-4, atol=1e-4)
  ref.check_paths(W, nf, table, labels, weights, log_z)
  steps, worst = ref.replay(W, nf, table, labels, seed, alpha)
  print(f'{name}: {steps} steps replayed, worst shortfall {worst:.3f} of the bound')
  assert steps == S * sum(nf)
  if B == 4:
    assert not labels[3].any() and not weights[3].any()  # num_frames = 0: the empty path


def test_exact_distribution(cuda):
  run = lambda context, W, nf, S, seed: _sample(context, W, nf, S, seed, cuda)[0]
  assert ref.distribution_units(run, 'bigram_v2_t4') <= 5


def test_arc_marginals(cuda):
  """Every arc's count among S = 4096 samples against S m, m the oracle's Log
  marginal: |count - S m| <= 5 (sqrt(S m (1 - m)) + 1)."""
  from oracle import oracle as orc  # test infrastructure only
  rng = np.random.default_rng(40)
  B, V, T, S = 2, 8, 40, 4096
  context = lt.contexts.FullNGram(vocab_size=V, context_size=1)
  table = ref.table_of(context)
  C = V + 1
  nf = np.array([T, 33])
  W = rng.standard_normal([B, T, C, V + 1]).astype(np.float32)
  labels, _, _ = _sample(context, W, nf.tolist(), S, 77, cuda)
  _, m = orc.den_grad(W, nf.astype(np.int32), V, 1)
  counts = np.zeros([B, T, C, V + 1], np.int64)
  q = np.zeros([B, S], np.int64)
  bb = np.arange(B)[:, None].repeat(S, 1)
  for t in range(T):
    y = labels[:, :, t]
    live = (t < nf)[:, None] & np.ones([B, S], bool)
    np.add.at(counts, (bb[live], t, q[live], y[live]), 1)
    q = np.where(live & (y > 0), table[q, np.maximum(y, 1) - 1], q)
  assert counts.sum() == S * nf.sum()
  units = ref.count_units(counts.reshape(-1), m.astype(np.float64).reshape(-1).clip(0, 1), S)
  print(f'arc marginals: worst count deviation {units:.2f} units')
  assert units <= 5


def test_determinism_and_sample_prefix(cuda):
  rng = np.random.default_rng(3)
  context = lt.contexts.FullNGram(vocab_size=32, context_size=1)
  B, T = 3, 50
  W = rng.standard_normal([B, T, 33, 33]).astype(np.float32)
  nf = [T, 31, 50]
  a = _sample(context, W, nf, 8, 99, cuda)
  b = _sample(context, W, nf, 8, 99, cuda)
  c = _sample(context, W, nf, 8, 100, cuda)
  d = _sample(context, W, nf, 32, 99, cuda)   # four workgroups an utterance
  e = _sample(context, W, nf, 3, 99, cuda)    # three sampling waves, a shallower ring
  np.testing.assert_array_equal(a[0], b[0])
  np.testing.assert_array_equal(a[1], b[1])
  assert (a[0] != c[0]).any()
  np.testing.assert_array_equal(a[0], d[0][:, :8])
  np.testing.assert_array_equal(a[1], d[1][:, :8])
  np.testing.assert_array_equal(a[0][:, :3], e[0])
  assert len({tuple(r) for r in d[0][0]}) > 1


def test_unsampled_and_masked_arcs(cuda):
  rng = np.random.default_rng(5)
  context = lt.contexts.FullNGram(vocab_size=3, context_size=1)
  table = ref.table_of(context)
  B, T, S = 3, 8, 64
  W = rng.standard_normal([B, T, 4, 4]).astype(np.float32)
  W[1] = -np.inf                        # no path at all: unsampled
  W[2, :, :, 2] = -np.inf               # label 2 masked everywhere
  W[2, 3, :, 0] = -np.inf               # and no blank on frame 3
  labels, weights, log_z = _sample(context, W, [T, T, T], S, 17, cuda)
  ref.check_paths(W, [T, T, T], table, labels, weights, log_z)
  assert log_z[1] == -np.inf and (weights[1] == -np.inf).all() and not labels[1].any()
  assert np.isfinite(weights[[0, 2]]).all()
  assert (labels[2] != 2).all() and (labels[2, :, 3] != 0).all()


def test_frame_label_dependent_raises(cuda):
  context = lt.contexts.FullNGram(vocab_size=3, context_size=1)
  lat = _lattice(context, torch.zeros([1, 4, 4, 4], device=cuda), K=2)
  with pytest.raises(NotImplementedError):
    lat.sample(torch.zeros([1, 4, 1], device=cuda), torch.tensor([4], device=cuda), 2, 0)


def test_abi_error_codes_and_workspace(cuda):
  """LT_EUNSUPPORTED for expansions >= 1 and LT_EINVAL for num_samples = 0,
  on real device buffers, with the outputs left untouched; the workspace
  query agrees with what the call accepts."""
  lib = nat.lib()
  V, T, B, S = 4, 6, 2, 3
  context = lt.contexts.FullNGram(vocab_size=V, context_size=1)
  W = torch.randn([B, T, V + 1, V + 1], device=cuda)
  nf = torch.tensor([T, 4], dtype=torch.int32, device=cuda)
  graph = nat.TableGraph(context.next_state_table(), 0, cuda)
  fld = nat.TableGraph(context.next_state_table(), 1, cuda)
  log_z, alpha = nat.table_forward(graph, W, nf, nat.SEMIRING_LOG)
  labels = torch.full([B, S, T], -7, dtype=torch.int64, device=cuda)
  weight = torch.full([B, S], -7.0, device=cuda)
  pb = nat.TableProblem(B, T, 0, nat.LT_DTYPE_F32)
  stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  ptr = lambda t: ctypes.c_void_p(t.data_ptr())

  def call(g, num_samples, ws=None, nbytes=0):
    return lib.lt_table_sample(ctypes.byref(g.g), ctypes.byref(pb), ptr(W), ptr(nf), ptr(log_z),
                               ptr(alpha), num_samples, 5, ptr(labels), ptr(weight), ws, nbytes,
                               stream)

  nbytes = ctypes.c_size_t(99)
  assert call(fld, S) == nat.LT_EUNSUPPORTED
  assert lib.lt_table_sample_workspace_bytes(ctypes.byref(fld.g), ctypes.byref(pb), S,
                                             ctypes.byref(nbytes)) == nat.LT_EUNSUPPORTED
  assert call(graph, 0) == -1
  assert lib.lt_table_sample_workspace_bytes(ctypes.byref(graph.g), ctypes.byref(pb), 0,
                                             ctypes.byref(nbytes)) == -1
  torch.cuda.synchronize()
  assert (labels == -7).all() and (weight == -7).all()  # nothing was launched
  assert lib.lt_table_sample_workspace_bytes(ctypes.byref(graph.g), ctypes.byref(pb), S,
                                             ctypes.byref(nbytes)) == 0
  ws = torch.empty([max(nbytes.value, 1)], dtype=torch.uint8, device=cuda)
  assert call(graph, S, ptr(ws) if nbytes.value else None, nbytes.value) == 0
  torch.cuda.synchronize()
  got, gw = nat.table_sample(graph, W, nf, log_z, alpha, S, 5)
  assert torch.equal(got, labels) and torch.equal(gw, weight)
  assert (labels >= 0).all() and (labels <= V).all() and not labels[1, :, 4:].any()
