"""RecognitionLattice.sampled_risk and path_weights on the GPU.

Everything is checked against the paths and costs the call itself returned
(path_ref, NumPy): the GPU's and the CPU's samplers may part on near-ties of
their two logf's, which the project reports rather than asserts.

* costs equal the reference edit distances of the returned alignment_labels,
  risk their mean, and the weight gradient the float64 scatter of
  adv = (c - mean c) / (S - 1) over the returned paths, within
  S 2^-24 sum_s |adv_s| per element -- on the tuned FullNGram route (bigram
  V = 32) and on the table route (C = 17), fp32 and bf16.
* The same seed gives the same outputs twice; the paths are `sample`'s.
* S = 1: the gradient is c (indicator - Log marginals), the marginals from
  `_forward`'s own backward, within the project's 1e-4 marginal bound.
* A custom cost_fn, batch dims [2, 2], an utterance with log_z = -inf (risk 0,
  zero gradient, no NaN), FrameLabelDependent.
"""
import numpy as np
import pytest
import torch

import last_torch_amd as lt
import path_ref
import sample_ref

pytestmark = pytest.mark.gpu

CONTEXTS = {
    'bigram_v32': lambda rng: lt.contexts.FullNGram(vocab_size=32, context_size=1),
    'table_c17_v6': lambda rng: lt.contexts.NextStateTable(sample_ref.random_table(rng, 17, 6)),
}
B, T, S, U = 4, 70, 5, 12
NF = [T, T - 3, 1, 0]


def _lattice(context, table, K=0):
  align = lt.alignments.FrameDependent() if K == 0 else lt.alignments.FrameLabelDependent(K)
  return lt.RecognitionLattice(
      context=context, alignment=align,
      weight_fn_cacher_factory=lambda _: lt.weight_fns.NullCacher(),
      weight_fn_factory=lambda _: lt.weight_fns.TableWeightFn(table))


def _frames(cuda, B=B, T=T):
  return torch.arange(T, dtype=torch.float32, device=cuda)[None, :, None].expand(B, T, 1)


def _problem(name, cuda, dtype=torch.float32):
  rng = np.random.default_rng(sum(map(ord, name)))
  context = CONTEXTS[name](rng)
  table = sample_ref.table_of(context)
  C, V = table.shape
  # a softer posterior than N(0, 1) logits: more blanks, hypotheses of varied length
  W = rng.standard_normal([B, T, C, V + 1]).astype(np.float32)
  W[..., 0] += 3.0
  Wd = torch.tensor(W).to(cuda, dtype).requires_grad_(True)
  ref = torch.tensor(rng.integers(1, V + 1, [B, U]).astype(np.int32), device=cuda)
  nl = torch.tensor([U, 7, 1, 0], device=cuda)
  return context, table, Wd, Wd.detach().float().cpu().numpy(), ref, nl


def _adv_scatter(W, nf, table, paths, costs, risk):
  """The float64 scatter of adv = (c - risk) / (S - 1), adv in fp32 as the
  method forms it (up to the ulp between a division and a multiplication by
  the reciprocal, which the S 2^-24 sum |adv| bound covers next to the S - 1
  adds of the sum)."""
  S = costs.shape[-1]
  adv = (costs - risk[:, None]) / np.float32(S - 1)
  states = path_ref.score(W, nf, table, paths)[3]
  return path_ref.scatter(W.shape, nf, paths, states, adv)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('name', list(CONTEXTS))
def test_risk_costs_and_gradient(cuda, name, dtype):
  context, table, Wd, W, ref, nl = _problem(name, cuda, dtype)
  lat = _lattice(context, Wd)
  nf = torch.tensor(NF, device=cuda)
  risk, costs, paths = lat.sampled_risk(_frames(cuda), nf, ref, nl, S, 11)
  assert risk.is_cuda and tuple(risk.shape) == (B,) and tuple(costs.shape) == (B, S)
  assert tuple(paths.shape) == (B, S, T) and paths.dtype == torch.int64
  assert costs.dtype == torch.float32 and not costs.requires_grad and risk.requires_grad
  p, c = paths.cpu().numpy(), costs.cpu().numpy()
  want = path_ref.edit_distance(p, NF, ref.cpu().numpy(), nl.cpu().numpy())[0]
  np.testing.assert_array_equal(c, want.astype(np.float32))
  assert len(np.unique(c[0])) > 1                         # the samples' costs differ
  # the mean: a sum of small integers (exact), then a division or a
  # multiplication by fl(1/S): two ulps apart at the most
  r = risk.detach().cpu().numpy()
  np.testing.assert_allclose(r, c.sum(-1) / S, rtol=2.5e-7, atol=0)
  # the paths are sample's, and they score to its weights
  labels, weights, _ = lat.sample(_frames(cuda), nf, S, 11)
  assert torch.equal(labels, paths)
  assert torch.equal(lat.path_weights(_frames(cuda), nf, paths).detach(), weights)
  risk.sum().backward()
  got = Wd.grad.float().cpu().numpy()
  dW, mag = _adv_scatter(W, NF, table, p, c, r)
  if dtype == torch.float32:
    assert (np.abs(got - dW) <= S * 2.0**-24 * mag).all()
  else:  # the fp32 scatter rounded once to bf16
    assert (np.abs(got - dW) <= S * 2.0**-24 * mag + 2.0**-8 * np.abs(dW)).all()
  assert not got[mag == 0].any() and got.any()
  # the same seed: the same outputs
  again = lat.sampled_risk(_frames(cuda), nf, ref, nl, S, 11)
  for x, y in zip((risk, costs, paths), again):
    assert torch.equal(x.detach(), y.detach())
  other = lat.sampled_risk(_frames(cuda), nf, ref, nl, S, 12)
  assert not torch.equal(other[2], paths)


@pytest.mark.parametrize('name', list(CONTEXTS))
def test_path_weights_gradient_and_second_backward(cuda, name):
  context, table, Wd, W, _, _ = _problem(name, cuda)
  lat = _lattice(context, Wd)
  rng = np.random.default_rng(2)
  nf = torch.tensor(NF, device=cuda)
  paths = lat.sample(_frames(cuda), nf, S, 4)[0]
  g = rng.integers(-3, 4, [B, S]).astype(np.float32)
  weights = lat.path_weights(_frames(cuda), nf, paths)
  w32, _, _, states = path_ref.score(W, NF, table, paths.cpu().numpy())
  np.testing.assert_array_equal(weights.detach().cpu().numpy(), w32)
  want, _ = path_ref.scatter(W.shape, NF, paths.cpu().numpy(), states, g)
  for _ in range(2):                                      # the second backward reuses the states
    Wd.grad = None
    weights.backward(torch.tensor(g, device=cuda), retain_graph=True)
    np.testing.assert_array_equal(Wd.grad.cpu().numpy(), want)


@pytest.mark.parametrize('name', list(CONTEXTS))
def test_single_sample_gradient(cuda, name):
  """S = 1: dR/dW = c (1[a in pi] - marginal_a), the marginals from the Log
  `_forward` backward on the same weights."""
  from last_torch_amd import semirings
  context, table, Wd, W, ref, nl = _problem(name, cuda)
  lat = _lattice(context, Wd)
  nf = torch.tensor(NF, device=cuda)
  risk, costs, paths = lat.sampled_risk(_frames(cuda), nf, ref, nl, 1, 21)
  assert torch.equal(risk.detach(), costs[:, 0])
  risk.sum().backward()
  got = Wd.grad.cpu().numpy()
  Wd.grad = None
  log_z, _ = lat._forward(None, _frames(cuda), nf, semirings.Log)
  log_z.sum().backward()
  marg = Wd.grad.cpu().numpy()
  p, c = paths.cpu().numpy(), costs.cpu().numpy()
  states = path_ref.score(W, NF, table, p)[3]
  ind, _ = path_ref.scatter(W.shape, NF, p, states, np.ones([B, 1]))
  want = c[:, 0, None, None, None] * (ind - marg)
  assert c[:2].min() > 0
  np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4 * c.max())


def test_custom_cost_and_batch_dims(cuda):
  context, table, Wd, W, ref, nl = _problem('table_c17_v6', cuda)
  lat = _lattice(context, Wd.detach().reshape(2, 2, *Wd.shape[1:]).requires_grad_(True))
  frames = _frames(cuda).reshape(2, 2, T, 1)
  nf = torch.tensor(NF, device=cuda).reshape(2, 2)
  seen = []

  def cost_fn(alignment_labels, num_frames):
    seen.append((tuple(alignment_labels.shape), tuple(num_frames.shape)))
    return (alignment_labels == 2).sum(-1).float()          # how often label 2 is emitted

  risk, costs, paths = lat.sampled_risk(frames, nf, None, None, S, 5, cost_fn=cost_fn)
  assert seen == [((2, 2, S, T), (2, 2))]
  assert tuple(risk.shape) == (2, 2) and tuple(costs.shape) == (2, 2, S)
  assert tuple(paths.shape) == (2, 2, S, T)
  p = paths.cpu().numpy().reshape(B, S, T)
  want = (p == 2).sum(-1).astype(np.float32)
  np.testing.assert_array_equal(costs.cpu().numpy().reshape(B, S), want)
  np.testing.assert_allclose(risk.detach().cpu().numpy().reshape(B), want.sum(-1) / S,
                             rtol=2.5e-7, atol=0)
  flat = _lattice(context, Wd).sampled_risk(_frames(cuda), nf.reshape(B), ref, nl, S, 5)
  np.testing.assert_array_equal(flat[2].cpu().numpy(), p)
  # default cost with batch dims
  risk2, costs2, _ = lat.sampled_risk(frames, nf, ref.reshape(2, 2, U), nl.reshape(2, 2), S, 5)
  np.testing.assert_array_equal(costs2.cpu().numpy().reshape(B, S), flat[1].cpu().numpy())


def test_unsampled_utterance_has_zero_risk_and_gradient(cuda):
  context, table, Wd, W, ref, nl = _problem('bigram_v32', cuda)
  with torch.no_grad():
    Wd[1] = -torch.inf                                     # every arc masked: log_z = -inf
  lat = _lattice(context, Wd)
  nf = torch.tensor(NF, device=cuda)
  for num_samples in (S, 1):
    Wd.grad = None
    risk, costs, paths = lat.sampled_risk(_frames(cuda), nf, ref, nl, num_samples, 3)
    assert risk[1] == 0 and not costs[1].any() and not paths[1].any()
    assert risk[0] > 0 and not torch.isnan(risk).any()
    risk.sum().backward()
    assert not torch.isnan(Wd.grad).any() and not Wd.grad[1].any() and Wd.grad[0].any()


def test_frame_label_dependent_raises(cuda):
  context = lt.contexts.FullNGram(vocab_size=3, context_size=1)
  lat = _lattice(context, torch.zeros([1, 4, 4, 4], device=cuda), K=2)
  frames, nf = torch.zeros([1, 4, 1], device=cuda), torch.tensor([4], device=cuda)
  with pytest.raises(NotImplementedError):
    lat.sampled_risk(frames, nf, torch.ones([1, 2], device=cuda).long(),
                     torch.tensor([2], device=cuda), 2, 0)
  with pytest.raises(NotImplementedError):
    lat.path_weights(frames, nf, torch.zeros([1, 2, 4], device=cuda).long())
