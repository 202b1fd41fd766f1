"""References for RecognitionLattice.expectation (include/lt_expect.h), shared
by tests/test_expectation_cpu.py and tests/test_gpu_expectation.py.

* enumerate_bigram: a float64 torch enumeration of every path of a small
  bigram lattice (each live frame takes label y in 0..V from state p: y = 0
  keeps p, y >= 1 moves to y; every state is final). p(pi) by logsumexp over
  the paths, E and H from it; gradients by autograd through the enumeration.
* cpu_reference: cpu.expectation in a chosen dtype (float64: the reference of
  the GPU tests; float32: the yardstick of cov's tolerance) with the gradients
  of (a * E + b * log_z).sum().
"""
import numpy as np
import torch

import last_torch_amd as lt
from last_torch_amd import cpu


def enumerate_bigram(W, values, nf):
  """W, values [B, T, V+1, V+1] float64 (may require grad), nf a list.
  Returns (E [B], log_z [B], H [B]); an utterance without a finite log_z
  gives E = H = 0 as constants."""
  B, T, C, R = W.shape
  Es, lzs, Hs = [], [], []
  for b in range(B):
    n = min(max(int(nf[b]), 0), T)
    if n == 0:
      ys = torch.zeros([1, 0], dtype=torch.long)
    else:
      ys = torch.cartesian_prod(*([torch.arange(R)] * n)).reshape(-1, n)
    st = [torch.zeros([ys.shape[0]], dtype=torch.long)]
    for t in range(n):
      st.append(torch.where(ys[:, t] == 0, st[-1], ys[:, t]))
    ps = torch.stack(st[:-1], dim=1) if n else ys
    ts = torch.arange(n)[None, :].expand_as(ys)
    w = W[b, ts, ps, ys].sum(dim=1)          # [P] path weights
    lz = torch.logsumexp(w, dim=0)
    if not torch.isfinite(lz):
      Es.append(torch.zeros([], dtype=W.dtype))
      Hs.append(torch.zeros([], dtype=W.dtype))
      lzs.append(lz.detach())
      continue
    on = w > -torch.inf
    p = torch.exp(w - lz)
    v = torch.where(on, values[b, ts, ps, ys].sum(dim=1), torch.zeros_like(w))
    Es.append((p * v).sum())
    logp = torch.where(on, w - lz, torch.zeros_like(w))
    Hs.append(-(p * logp).sum())
    lzs.append(lz)
  return torch.stack(Es), torch.stack(lzs), torch.stack(Hs)


def grads(E, log_z, inputs, a=None, b=None):
  """Gradients of (a * E + b * log_z).sum() w.r.t. `inputs` (zeros for an
  input the loss does not reach)."""
  a = torch.ones_like(E) if a is None else a.to(E.dtype)
  b = torch.ones_like(log_z) if b is None else b.to(E.dtype)
  # log_z = -inf utterances carry no gradient (and inf * 0 would be NaN)
  lz = torch.where(torch.isfinite(log_z), log_z, torch.zeros_like(log_z))
  loss = (a * E + b * lz).sum()
  out = torch.autograd.grad(loss, inputs, allow_unused=True)
  return [torch.zeros_like(x) if g is None else g for x, g in zip(inputs, out)]


def cpu_reference(W, values, nf, context, a=None, b=None, dtype=torch.float64):
  """cpu.expectation in `dtype` on the host: dict of float64 numpy arrays E,
  log_z, dW, dv for the loss (a * E + b * log_z).sum()."""
  Wd = W.detach().cpu().to(dtype).requires_grad_(True)
  vd = values.detach().cpu().to(dtype).requires_grad_(True)
  E, log_z = cpu.expectation(Wd, vd, torch.as_tensor(nf).long(), context)
  a = None if a is None else a.detach().cpu()
  b = None if b is None else b.detach().cpu()
  dW, dv = grads(E, log_z, [Wd, vd], a, b)
  return {k: x.detach().double().numpy() for k, x in
          (('E', E), ('log_z', log_z), ('dW', dW), ('dv', dv))}


def table_lattice(context, table, K=0):
  align = lt.alignments.FrameDependent() if K == 0 else lt.alignments.FrameLabelDependent(K)
  return lt.RecognitionLattice(
      context=context, alignment=align,
      weight_fn_cacher_factory=lambda _: lt.weight_fns.NullCacher(),
      weight_fn_factory=lambda _: lt.weight_fns.TableWeightFn(table))


def frames(batch_dims, T, device='cpu'):
  """Frames whose single feature is the row t of a TableWeightFn table."""
  return torch.arange(T, dtype=torch.float32, device=device)[:, None].expand(*batch_dims, T, 1)


def random_table(rng, C, V, sinks=()):
  """A random next-state table [C, V] (int32 tensor); for every pair (y, q)
  of `sinks` each arc of label index y goes to state q (a state of large
  in-degree)."""
  tab = rng.integers(0, C, size=[C, V]).astype(np.int32)
  for y, q in sinks:
    tab[:, y] = q
  return torch.from_numpy(tab)
