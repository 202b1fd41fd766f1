"""The independent reference for RecognitionLattice.align_posteriors -- TEST
INFRASTRUCTURE, shared by tests/test_align_post_cpu.py and
tests/test_gpu_align_post.py.

Built only from what the package had before the method existed:
cpu.string_weights, then cpu._string_distance(..., semirings.Log),
differentiated with respect to the string's own lexical weights. It does not
call cpu.align_posteriors. In float64 it is the reference; the same function
in float32 is the yardstick the tolerances are taken from.
"""
import torch

import last_torch_amd as lt
from last_torch_amd import cpu


def reference(W, nf, labels, nl, context, K=0, dtype=torch.float64):
  """(emission [B, T, U], log_prob [B]) in `dtype` on the host. Labels must
  lie in 0..V (0: epsilon). An utterance whose distance is not finite is
  masked out of the differentiated sum: log_prob = -inf, emission 0."""
  W = torch.as_tensor(W).detach().cpu().to(dtype)
  lab = torch.as_tensor(labels).cpu().long()
  nf = torch.as_tensor(nf).cpu().long()
  nl = torch.as_tensor(nl).cpu().long()
  B, T = W.shape[:2]
  U = lab.shape[-1]
  with torch.enable_grad():
    blank, lex = cpu.string_weights(W, lab, context)
    lex = lex.detach().requires_grad_(True)
    dist = cpu._string_distance(blank, lex, nf, nl, K, lt.semirings.Log)
    fin = torch.isfinite(dist.detach())
    total = torch.where(fin, dist, torch.zeros_like(dist)).sum()
    grad = (torch.autograd.grad(total, [lex], allow_unused=True)[0]
            if total.requires_grad else None)
  dist = dist.detach()
  emission = torch.zeros([B, T, U], dtype=dtype)
  if grad is not None:
    emission = torch.where(fin[:, None, None], grad, emission)
  return emission, torch.where(fin, dist, torch.full_like(dist, -torch.inf))


def yardstick(W, nf, labels, nl, context, K=0):
  """(emission error, log_prob error, float64 emission, float64 log_prob):
  the max abs error of the float32 run of `reference` against its float64 run,
  over the utterances both align (log_prob: finite entries)."""
  e64, l64 = reference(W, nf, labels, nl, context, K, torch.float64)
  e32, l32 = reference(W, nf, labels, nl, context, K, torch.float32)
  fin = torch.isfinite(l64)
  assert torch.equal(fin, torch.isfinite(l32))
  e_err = float((e32.double() - e64).abs().max()) if e64.numel() else 0.0
  l_err = float((l32.double() - l64)[fin].abs().max()) if fin.any() else 0.0
  return e_err, l_err, e64, l64
