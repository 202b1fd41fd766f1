"""Forced alignment on the GPU (RecognitionLattice.align -> lt_table_align,
lt_align.hip): alignment_labels, label_frames and path_weights, all exact,
against

* the reference's own autograd through _string_forward in MaxTropical
  (tests/golden/grads_*.npz) on every FrameDependent / FrameLabelDependent
  fixture, compacted by align_compact.compact;
* the pinned C oracle (table_oracle.c tab_dist_grad, itself checked against
  those fixtures by tests/test_oracle_grads.py) on random problems at the
  kernel's lane and slice boundaries (U = 63 .. 255), with integer weights
  (ties everywhere) and Gaussian ones, ragged lengths, unaligned utterances,
  epsilon labels, a trigram, a random next-state table, bf16 weights,
  FrameLabelDependent(K), and decisions that do not fit LDS.
"""
import zlib

import numpy as np
import pytest
import torch

import last_torch_amd as lt
from last_torch_amd import _native as nat
from align_compact import CASES, compact, load

pytestmark = pytest.mark.gpu


def _orc():
  from oracle import oracle as orc  # test infrastructure only
  return orc


def _lattice(context, K, table):
  align = lt.alignments.FrameDependent() if K == 0 else lt.alignments.FrameLabelDependent(K)
  return lt.RecognitionLattice(
      context=context, alignment=align,
      weight_fn_cacher_factory=lambda _: lt.weight_fns.NullCacher(),
      weight_fn_factory=lambda _: lt.weight_fns.TableWeightFn(table))


def _frames(batch, T, device):
  return torch.arange(T, dtype=torch.float32, device=device)[:, None].expand(*batch, T, 1)


def _align(lat, W, nf, lab, nl, device):
  """RecognitionLattice.align on ROCm tensors, as numpy."""
  B, T = W.shape[:2]
  out = lat.align(_frames((B,), T, device), torch.tensor(nf, device=device),
                  torch.tensor(lab, device=device), torch.tensor(nl, device=device))
  return [x.cpu().numpy() for x in out]


def _assert_equal(got, ref_labels, ref_frames, ref_dist):
  labels, frames, dist = got
  assert labels.dtype == np.int64 and frames.dtype == np.int64 and dist.dtype == np.float32
  np.testing.assert_array_equal(dist, ref_dist)
  np.testing.assert_array_equal(labels, ref_labels)
  np.testing.assert_array_equal(frames, ref_frames)


@pytest.mark.parametrize('name', CASES)
def test_align_matches_reference_autograd(cuda, name):
  d = load(name)
  V, n, K = int(d['vocab_size']), int(d['context_size']), d['K']
  ref_labels, ref_frames = compact(d['num_grad_MaxTropical'], d['num_MaxTropical'], d['labels'],
                                   d['num_labels'], d['num_frames'], K)
  lat = _lattice(lt.contexts.FullNGram(vocab_size=V, context_size=n), K,
                 torch.tensor(d['W'], device=cuda))
  got = _align(lat, d['W'], d['num_frames'], d['labels'], d['num_labels'], cuda)
  _assert_equal(got, ref_labels, ref_frames, d['num_MaxTropical'])


def _weights(rng, kind, shape):
  if kind == 'ints':  # ties everywhere
    return rng.integers(-3, 4, shape).astype(np.float32)
  return rng.standard_normal(shape).astype(np.float32)


def _lengths(rng, T, U, K):
  """Four utterances: full length with num_labels = U; full length with the
  longest string the frames carry (less a little); empty; three frames with
  one label too many (unaligned)."""
  per = max(K, 1)
  nf = np.array([T, T, 0, 3], np.int32)
  nl = np.array([U, max(0, min(U, T * per) - int(rng.integers(0, 4))), 0, min(U, 3 * per + 1)],
                np.int32)
  assert nl[3] > nf[3] * per
  return nf, nl


RANDOM = [
    # name, V, n (FullNGram) or None (random table of C states), C, K, T, U, dtype, epsilon
    ('bigram_u63', 32, 1, None, 0, 70, 63, 'f32', False),
    ('bigram_u64', 32, 1, None, 0, 70, 64, 'f32', False),
    ('bigram_u65', 32, 1, None, 0, 70, 65, 'f32', False),
    ('bigram_u127', 32, 1, None, 0, 70, 127, 'f32', False),
    ('bigram_u128', 32, 1, None, 0, 70, 128, 'f32', False),
    ('bigram_u255', 32, 1, None, 0, 70, 255, 'f32', False),
    ('trigram_v5_eps', 5, 2, None, 0, 30, 9, 'f32', True),
    ('table_c17_v6', 6, None, 17, 0, 30, 9, 'f32', True),
    ('table_c300_v28', 28, None, 300, 0, 20, 9, 'f32', True),  # too large to stage in LDS
    ('bigram_bf16_u65', 32, 1, None, 0, 70, 65, 'bf16', False),
    ('fld_k1', 4, 1, None, 1, 20, 12, 'f32', False),
    ('fld_k2', 4, 1, None, 2, 20, 12, 'f32', False),
    ('fld_k3', 4, 1, None, 3, 20, 12, 'f32', True),
    ('fld_k2_v32_u65', 32, 1, None, 2, 40, 65, 'f32', False),
]


def _problem(case, kind):
  name, V, n, C, K, T, U, dt, eps = case
  orc = _orc()
  rng = np.random.default_rng(zlib.crc32(f'{name}-{kind}'.encode()))
  if n is not None:
    ctx = lt.contexts.FullNGram(vocab_size=V, context_size=n)
    tab = orc.full_ngram_table(V, n)
  else:
    tab = rng.integers(0, C, (C, V)).astype(np.int32)
    ctx = lt.contexts.NextStateTable(torch.tensor(tab))
  B = 4
  W = _weights(rng, kind, (B, T, tab.shape[0], V + 1))
  if dt == 'bf16':
    W = torch.tensor(W).bfloat16().float().numpy()
  nf, nl = _lengths(rng, T, U, K)
  lab = rng.integers(0 if eps else 1, V + 1, (B, U)).astype(np.int32)
  return ctx, tab, W, nf, lab, nl


@pytest.mark.parametrize('case', RANDOM, ids=[c[0] for c in RANDOM])
@pytest.mark.parametrize('kind', ['ints', 'gauss'])
def test_align_random_against_oracle(cuda, case, kind):
  orc = _orc()
  K, dt = case[4], case[7]
  ctx, tab, W, nf, lab, nl = _problem(case, kind)
  rd, rg = orc.tab_dist_grad(tab, W, nf, K, orc.MAX, lab, nl)
  ref_labels, ref_frames = compact(rg, rd, lab, nl, nf, K)
  assert np.isfinite(rd[1:3]).all() and rd[3] == -np.inf and (ref_frames[3] == -1).all()
  lat = _lattice(ctx, K, torch.tensor(W, device=cuda))
  if dt == 'bf16':
    # TableWeightFn hands out fp32: the bf16 kernel through the binding
    out = nat.table_align(lat._graph(cuda), torch.tensor(W, device=cuda).bfloat16().contiguous(),
                          torch.tensor(nf, device=cuda), torch.tensor(lab, device=cuda),
                          torch.tensor(nl, device=cuda))
    got = [x.cpu().numpy() for x in out]
  else:
    got = _align(lat, W, nf, lab, nl, cuda)
  _assert_equal(got, ref_labels, ref_frames, rd)


@pytest.mark.parametrize('T,kind', [(2500, 'ints'), (5200, 'ints'), (5200, 'gauss')])
def test_align_decisions_beyond_lds(cuda, T, kind):
  """5200 x 256 decision bits exceed 160 KiB: the decisions go through the
  workspace and come back in staged chunks. (2500 frames of them still fit,
  in more than the 64 KiB of LDS a kernel has by default.)"""
  orc = _orc()
  V, U = 4, 255
  rng = np.random.default_rng(zlib.crc32(f'deep-{T}-{kind}'.encode()))
  tab = orc.full_ngram_table(V, 1)
  W = _weights(rng, kind, (2, T, tab.shape[0], V + 1))
  nf = np.array([T, 37], np.int32)
  nl = np.array([255, 20], np.int32)
  lab = rng.integers(1, V + 1, (2, U)).astype(np.int32)
  rd, rg = orc.tab_dist_grad(tab, W, nf, 0, orc.MAX, lab, nl)
  assert np.isfinite(rd).all()
  ref_labels, ref_frames = compact(rg, rd, lab, nl, nf, 0)
  lat = _lattice(lt.contexts.FullNGram(vocab_size=V, context_size=1), 0,
                 torch.tensor(W, device=cuda))
  _assert_equal(_align(lat, W, nf, lab, nl, cuda), ref_labels, ref_frames, rd)


def test_align_weights_resum_in_frame_order(cuda):
  """The returned alignment alone gives back path_weights: its W entries
  summed in frame order in fp32, bit for bit."""
  case = next(c for c in RANDOM if c[0] == 'bigram_u65')
  ctx, tab, W, nf, lab, nl = _problem(case, 'gauss')
  lat = _lattice(ctx, 0, torch.tensor(W, device=cuda))
  labels, frames, dist = _align(lat, W, nf, lab, nl, cuda)
  checked = 0
  for b in range(W.shape[0]):
    if not dist[b] > -np.inf:
      continue
    acc, c, u = np.float32(0), 0, 0
    for t in range(int(nf[b])):
      y = int(labels[b, t])
      if y:
        assert y == lab[b, u] and frames[b, u] == t
        acc = np.float32(acc + W[b, t, c, y])
        c, u = int(tab[c, y - 1]), u + 1
      else:
        acc = np.float32(acc + W[b, t, c, 0])
    assert u == nl[b]
    assert acc == dist[b], (b, acc, dist[b])
    checked += 1
  assert checked >= 3


def test_align_fallback_beyond_kernel_range(cuda):
  """U = 300 is past the kernel: the binding refuses (LT_EUNSUPPORTED) and
  RecognitionLattice.align answers through the dense route."""
  orc = _orc()
  V, T, U, B = 8, 320, 300, 2
  rng = np.random.default_rng(77)
  tab = orc.full_ngram_table(V, 1)
  W = _weights(rng, 'ints', (B, T, tab.shape[0], V + 1))
  nf = np.array([320, 200], np.int32)
  nl = np.array([300, 120], np.int32)
  lab = rng.integers(1, V + 1, (B, U)).astype(np.int32)
  rd, rg = orc.tab_dist_grad(tab, W, nf, 0, orc.MAX, lab, nl)
  ref_labels, ref_frames = compact(rg, rd, lab, nl, nf, 0)
  lat = _lattice(lt.contexts.FullNGram(vocab_size=V, context_size=1), 0,
                 torch.tensor(W, device=cuda))
  _assert_equal(_align(lat, W, nf, lab, nl, cuda), ref_labels, ref_frames, rd)
  with pytest.raises(nat.LatticeLibraryError, match=r'\(-2\)'):
    nat.table_align(lat._graph(cuda), torch.tensor(W, device=cuda), torch.tensor(nf, device=cuda),
                    torch.tensor(lab, device=cuda), torch.tensor(nl, device=cuda))


def test_align_dense_route_agrees_inside_kernel_range(cuda):
  """_align_dense, the fallback and the timing baseline, gives the kernel's
  answer where both run (FrameLabelDependent slots included)."""
  for name in ('bigram_u65', 'fld_k2_v32_u65'):
    case = next(c for c in RANDOM if c[0] == name)
    ctx, tab, W, nf, lab, nl = _problem(case, 'ints')
    lat = _lattice(ctx, case[4], torch.tensor(W, device=cuda))
    args = (lat._graph(cuda), torch.tensor(W, device=cuda), torch.tensor(nf, device=cuda),
            torch.tensor(lab, device=cuda), torch.tensor(nl, device=cuda))
    for x, y in zip(nat.table_align(*args), lat._align_dense(*args)):
      np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy())


def test_align_weights_equal_string_forward_with_batch_dims(cuda):
  """path_weights = _string_forward(..., MaxTropical) on batch dims [2, 3]."""
  V, T, U = 5, 25, 7
  rng = np.random.default_rng(3)
  ctx = lt.contexts.FullNGram(vocab_size=V, context_size=1)
  W = torch.tensor(rng.standard_normal((2, 3, T, ctx.num_states(), V + 1)).astype(np.float32),
                   device=cuda)
  lat = _lattice(ctx, 0, W)
  frames = _frames((2, 3), T, cuda)
  nf = torch.tensor([[25, 10, 0], [3, 25, 17]], device=cuda)
  nl = torch.tensor([[7, 3, 0], [5, 0, 7]], device=cuda)
  lab = torch.tensor(rng.integers(1, V + 1, (2, 3, U)), device=cuda)
  labels, lframes, weights = lat.align(frames, nf, lab, nl)
  assert tuple(labels.shape) == (2, 3, T) and tuple(lframes.shape) == (2, 3, U)
  assert tuple(weights.shape) == (2, 3) and weights.device == frames.device
  ref = lat._string_forward(None, frames, nf, lab, nl, lt.semirings.MaxTropical)
  np.testing.assert_array_equal(weights.cpu().numpy(), ref.cpu().numpy())
  assert weights[1, 0] == -torch.inf and (lframes[1, 0] == -1).all()  # 5 labels, 3 frames
  with pytest.raises(ValueError):
    lat.align(frames, nf, lab[0], nl)
