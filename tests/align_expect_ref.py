"""The independent reference for RecognitionLattice.align_expectation -- TEST
INFRASTRUCTURE, shared by tests/test_align_expect_cpu.py and
tests/test_gpu_align_expect.py.

Built only from what the package had before the method existed:
cpu.string_weights, then cpu._string_distance(..., semirings.Log),
differentiated twice by autograd. It does not call cpu.align_expectation. In
float64 it is the reference; the same function in float32 is the yardstick
the tolerances are taken from. `enumerate_alignments` is a second, direct
reference: every alignment of a short string, one by one.
"""
import itertools

import torch

import last_torch_amd as lt
from last_torch_amd import cpu

KEYS = ('expected', 'log_prob', 'emission', 'blank_occ', 'cov_lex', 'cov_blank', 'dW_expected',
        'dW_log_prob')


def reference(W, nf, labels, nl, context, lexical_values, blank_values, K=0, dtype=torch.float64):
  """A dict of host tensors in `dtype`:
    expected, log_prob [B]
    emission [B,T,U], blank_occ [B,T,U+1]   d log_prob / d (lex, blank)
    cov_lex [B,T,U], cov_blank [B,T,U+1]    d expected / d (lex, blank)
    dW_expected, dW_log_prob [B,T,C,V+1]    the dense gradients w.r.t. W
  (lex, blank) the string's own weights. Labels must lie in 0..V (0: epsilon).
  An utterance whose distance is not finite is masked out of every
  differentiated sum: log_prob = -inf, everything else 0. A value whose
  posterior is 0 is not read (NaN there is harmless)."""
  W = torch.as_tensor(W).detach().cpu().to(dtype).requires_grad_(True)
  lab = torch.as_tensor(labels).cpu().long()
  nf = torch.as_tensor(nf).cpu().long()
  nl = torch.as_tensor(nl).cpu().long()
  lv = torch.as_tensor(lexical_values).detach().cpu().to(dtype)
  bv = torch.as_tensor(blank_values).detach().cpu().to(dtype)
  B, T = W.shape[:2]
  U = lab.shape[-1]
  zero = lambda *shape: torch.zeros(shape, dtype=dtype)
  with torch.enable_grad():
    blank, lex = cpu.string_weights(W, lab, context)
    dist = cpu._string_distance(blank, lex, nf, nl, K, lt.semirings.Log)
    fin = torch.isfinite(dist.detach())
    total = torch.where(fin, dist, torch.zeros_like(dist)).sum()
    if not total.requires_grad:  # no frames at all
      em, bo, cl, cb = zero(B, T, U), zero(B, T, U + 1), zero(B, T, U), zero(B, T, U + 1)
      return dict(expected=zero(B), log_prob=torch.where(fin, dist.detach(), -torch.inf),
                  emission=em, blank_occ=bo, cov_lex=cl, cov_blank=cb,
                  dW_expected=torch.zeros_like(W), dW_log_prob=torch.zeros_like(W))
    em, bo = torch.autograd.grad(total, [lex, blank], create_graph=True)
    expected = ((em * torch.where(em.detach() != 0, lv, torch.zeros_like(lv))).sum((1, 2)) +
                (bo * torch.where(bo.detach() != 0, bv, torch.zeros_like(bv))).sum((1, 2)))
    cl, cb, dwe = torch.autograd.grad(expected.sum(), [lex, blank, W], retain_graph=True,
                                      allow_unused=True)
    (dwl,) = torch.autograd.grad(total, [W])
  fill = lambda g, like: torch.zeros_like(like) if g is None else g
  return dict(expected=expected.detach(),
              log_prob=torch.where(fin, dist.detach(), torch.full_like(dist, -torch.inf).detach()),
              emission=em.detach(), blank_occ=bo.detach(), cov_lex=fill(cl, lex).detach(),
              cov_blank=fill(cb, blank).detach(), dW_expected=fill(dwe, W).detach(),
              dW_log_prob=dwl.detach())


def yardstick(W, nf, labels, nl, context, lexical_values, blank_values, K=0):
  """(r64, err): the float64 reference and, per key of KEYS, the max abs error
  of the float32 run of `reference` against it (log_prob: finite entries)."""
  args = (W, nf, labels, nl, context, lexical_values, blank_values, K)
  r64 = reference(*args, dtype=torch.float64)
  r32 = reference(*args, dtype=torch.float32)
  fin = torch.isfinite(r64['log_prob'])
  assert torch.equal(fin, torch.isfinite(r32['log_prob']))
  err = {}
  for k in KEYS:
    d = (r32[k].double() - r64[k]).abs()
    if k == 'log_prob':
      d = d[fin]
    err[k] = float(d.max()) if d.numel() else 0.0
  return r64, err


def enumerate_alignments(W, labels, lexical_values, blank_values, context):
  """One utterance, every frame live and every label used: W [T, C, V+1],
  labels [U] in 1..V, values [T, U] / [T, U+1]. Visits each of the C(T, U)
  alignments (the frames on which the labels are emitted) and returns
  (expected, log_prob, entropy) as differentiable scalars."""
  T, U = W.shape[0], labels.shape[0]
  ctx = context.walk_states(labels[None].long())[0].tolist()
  lab = labels.tolist()
  ws, vs = [], []
  for frames in itertools.combinations(range(T), U):
    u, w, v = 0, W.new_zeros([]), W.new_zeros([])
    for t in range(T):
      if u < U and frames[u] == t:
        w, v, u = w + W[t, ctx[u], lab[u]], v + lexical_values[t, u], u + 1
      else:
        w, v = w + W[t, ctx[u], 0], v + blank_values[t, u]
    ws.append(w)
    vs.append(v)
  ws, vs = torch.stack(ws), torch.stack(vs)
  log_prob = torch.logsumexp(ws, 0)
  p = torch.exp(ws - log_prob)
  return (p * vs).sum(), log_prob, -(p * (ws - log_prob)).sum()


def lattice(context, K, table):
  """A lattice whose arc weights are rows of `table` [B, T, C, V+1]
  (TableWeightFn: frame t reads row t)."""
  align = lt.alignments.FrameDependent() if K == 0 else lt.alignments.FrameLabelDependent(K)
  return lt.RecognitionLattice(
      context=context, alignment=align,
      weight_fn_cacher_factory=lambda _: lt.weight_fns.NullCacher(),
      weight_fn_factory=lambda _: lt.weight_fns.TableWeightFn(table))


def frames(batch, T, device='cpu'):
  return torch.arange(T, dtype=torch.float32, device=device)[:, None].expand(*batch, T, 1)
