"""lt_edit_distance on the GPU (lt_edit.hip), exact against path_ref's
two-row Levenshtein.

U in {0, 1, 63, 64, 65, 127, 128, 255, 256, 300} (every cells-per-lane
instantiation and the lane-block boundaries around them, plus 600 and 1023 for
the two widest) crossed with T in {1, 64, 65, 130} (the 64-frame loads'
boundaries), B = 3, S = 4, tokens from a 3-symbol alphabet so that matches and
ties are frequent. Also: all-blank hypotheses, hypotheses equal to their
reference, zeros inside the reference, ragged num_frames / num_labels with 0
and out-of-range values, a missing num_frames, a second workgroup per
utterance, tokens past int32, and one reference past the kernel's range,
which last_torch_amd.edit_distance runs through the torch restatement on the
device.
"""
import numpy as np
import pytest
import torch

import last_torch_amd as lt
from last_torch_amd import _native as nat
import path_ref

pytestmark = pytest.mark.gpu


def _check(cuda, hyp, nf, ref, nl):
  d = lambda x, dt: None if x is None else torch.tensor(np.asarray(x), dtype=dt, device=cuda)
  dist, length = nat.edit_distance(d(hyp, torch.int64), d(nf, torch.int32), d(ref, torch.int32),
                                   d(nl, torch.int32))
  assert dist.dtype == torch.int32 and length.dtype == torch.int32
  want_d, want_l = path_ref.edit_distance(hyp, nf, ref, nl)
  np.testing.assert_array_equal(dist.cpu().numpy(), want_d)
  np.testing.assert_array_equal(length.cpu().numpy(), want_l)
  pub = lt.edit_distance(d(hyp, torch.int64), d(nf, torch.int32), d(ref, torch.int32),
                         d(nl, torch.int32))
  assert pub.is_cuda and pub.dtype == torch.int32
  np.testing.assert_array_equal(pub.cpu().numpy(), want_d)
  return want_d


@pytest.mark.parametrize('T', [1, 64, 65, 130])
@pytest.mark.parametrize('U', [0, 1, 63, 64, 65, 127, 128, 255, 256, 300])
def test_against_the_reference(cuda, U, T):
  rng = np.random.default_rng(1000 * U + T)
  B, S = 3, 4
  hyp = rng.integers(0, 4, [B, S, T])
  hyp[0, 1] = 0                                            # an all-blank hypothesis
  ref = rng.integers(0, 4, [B, U]).astype(np.int32)        # zeros inside the reference
  if U:
    n = min(U, T)
    hyp[1, 2] = 0
    hyp[1, 2, :n] = ref[1, :n]                             # a hypothesis equal to (a prefix of) ref
  d = _check(cuda, hyp, [T, T, T], ref, [U, U, U])
  if U and U <= T:
    assert d[1, 2] == 0
  _check(cuda, hyp, [T, T - 1, 0], ref, [U, max(U - 1, 0), U // 2])   # ragged
  _check(cuda, hyp, None, ref, [0, U + 1, -1])             # empty / out-of-range references


@pytest.mark.parametrize('U', [600, 1023])
def test_widest_instantiations(cuda, U):
  rng = np.random.default_rng(U)
  B, S, T = 2, 9, 130                                      # 9 hypotheses: two workgroups
  hyp = rng.integers(0, 4, [B, S, T])
  ref = rng.integers(1, 4, [B, U]).astype(np.int32)
  hyp[0, 3, :100] = ref[0, U - 100:]                       # matches at the far end of the row
  _check(cuda, hyp, [T, 77], ref, [U, U - 5])


def test_tokens_past_int32_match_nothing(cuda):
  hyp = np.array([[[5, 1 << 33, 0, (1 << 32) + 5, 7]]])
  ref = np.array([[5, 5, 7]], np.int32)
  d = _check(cuda, hyp, [5], ref, [3])
  assert d[0, 0] == 2


def test_reference_past_the_kernels_range_runs_the_torch_route(cuda):
  rng = np.random.default_rng(3)
  B, S, T, U = 2, 2, 40, 1024
  assert nat.edit_distance_supported(U - 1) and not nat.edit_distance_supported(U)
  hyp = rng.integers(0, 4, [B, S, T])
  ref = rng.integers(0, 4, [B, U]).astype(np.int32)
  nl = [U, 30]
  with pytest.raises(nat.LatticeLibraryError):
    nat.edit_distance(torch.tensor(hyp, device=cuda), None, torch.tensor(ref, device=cuda),
                      torch.tensor(nl, device=cuda))
  got = lt.edit_distance(torch.tensor(hyp, device=cuda), torch.tensor([T, 33], device=cuda),
                         torch.tensor(ref, device=cuda), torch.tensor(nl, device=cuda))
  assert got.is_cuda and got.dtype == torch.int32
  np.testing.assert_array_equal(got.cpu().numpy(),
                                path_ref.edit_distance(hyp, [T, 33], ref, nl)[0])


def test_batch_dims(cuda):
  rng = np.random.default_rng(4)
  hyp = rng.integers(0, 4, [2, 2, 3, 20])
  ref = rng.integers(0, 4, [2, 2, 6]).astype(np.int32)
  nf, nl = np.array([[20, 3], [0, 11]]), np.array([[6, 2], [5, 0]])
  got = lt.edit_distance(torch.tensor(hyp, device=cuda), torch.tensor(nf, device=cuda),
                         torch.tensor(ref, device=cuda), torch.tensor(nl, device=cuda))
  assert tuple(got.shape) == (2, 2, 3)
  want = path_ref.edit_distance(hyp.reshape(4, 3, 20), nf.reshape(-1), ref.reshape(4, 6),
                                nl.reshape(-1))[0]
  np.testing.assert_array_equal(got.cpu().numpy().reshape(4, 3), want)
