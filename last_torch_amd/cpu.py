"""PyTorch CPU path of the lattice algorithms, for CPU tensors.

``RecognitionLattice`` runs here when its arc weights live on the CPU and on
the HIP kernels (liblt_lattice.so) when they live on a ROCm device: the
device of the tensors picks the implementation, as in the reference, and
there is no fallback from one to the other (a ROCm tensor never runs on the
host; a missing HIP library raises). The functions here that also take ROCm
tensors are align_posteriors, align_expectation, path_weights, beam_search
and edit_distance, which then run their torch ops on that device:
RecognitionLattice.align_posteriors, align_expectation, path_weights and
beam_search and last_torch_amd.edit_distance past their kernels' range.

One formulation covers both alignment lattices and any context dependency.
A frame of FrameDependent (K = 0) or FrameLabelDependent(K) is

    alpha' = (+)_{i=0..max(K,1)} term_i,   term_0 = alpha (x) blank,
    K = 0:   term_1 = L(alpha)
    K >= 1:  term_i = L^i(alpha) (x) blank

with L the lexical step (the context's forward_reduce: a semiring sum over
each state's in-arcs) or, on the label string, one position shift
(alignments.py:286-297, 320-329, 363-377, 421-432; alignment-state-invariant
weights, lattices.py:444-447). The loop runs over frames vectorised over the
batch and the states; gradients are torch autograd through the semirings'
sound derivatives (semirings.py). The terms are summed in the order above, so
MaxTropical's first-argmax rule prefers the blank, then fewer expansions.

  den_forward   lattices.py:379-496   shortest distance + alpha_0..T-1
  num_forward   lattices.py:250-377   string (numerator) distance
  loss          lattices.py:131-183   log_z - num (or -num, locally normalised)
  viterbi       lattices.py:185-247   max-tropical distance, labels from its
                                      derivative w.r.t. one zero lexical mask
                                      per expansion
  align         (not in the reference) forced alignment: the max-tropical
                                      string distance differentiated w.r.t.
                                      the string's lexical weights
  align_posteriors (not in the reference) emission posteriors of the label
                                      string: the Log string distance
                                      differentiated w.r.t. the same weights
  align_expectation (not in the reference) posterior mean, over the string's
                                      alignments, of a path value in string
                                      coordinates (lt_string_expect.h): the
                                      same derivative kept in the graph
  sample        (not in the reference) paths from the posterior exp(w) / Z:
                                      Gumbel-max on Philox4x32-10, walked
                                      backwards over alpha (lt_sample.h)
  path_weights  (not in the reference) the weight of given paths (lt_paths.h):
                                      a table walk and a gather, summed from
                                      the last frame to the first as
                                      lt_sample.h does; plain autograd
  edit_distance (not in the reference) Levenshtein distance of the tokens of
                                      hypotheses against references
                                      (lt_paths.h), one DP row per token
  beam_search   (not in the reference) the N best label sequences by prefix
                                      beam search (lt_beam.h): one gather,
                                      merge and stable sort per frame
  expectation   (not in the reference) posterior mean of an arc-additive path
                                      value (lt_expect.h): the arc marginals
                                      by autograd with a graph, so the result
                                      is differentiable by ordinary autograd
"""
import torch

from last_torch_amd import alignments
from last_torch_amd import contexts
from last_torch_amd import semirings


def expansions(alignment) -> int:
  """K: 0 for FrameDependent, max_expansions for FrameLabelDependent."""
  if isinstance(alignment, alignments.FrameLabelDependent):
    return int(alignment.max_expansions)
  if isinstance(alignment, alignments.FrameDependent):
    return 0
  raise NotImplementedError('the CPU lattice path implements FrameDependent and '
                            f'FrameLabelDependent alignments; got {type(alignment).__name__}')


def _live(nf: torch.Tensor, t: int) -> torch.Tensor:
  return (t < nf)[:, None]


def _frame(alpha, step, blank, K, semiring):
  """One frame: (+) of the terms in the module docstring; `step(x, i)` is
  the i-th lexical step (0-based) applied to x."""
  terms = [semiring.times(alpha, blank)]
  last = alpha
  for i in range(max(K, 1)):
    last = step(last, i)
    terms.append(semiring.times(last, blank) if K else last)
  return semiring.sum(torch.stack(terms), dim=0)


def den_forward(W: torch.Tensor, nf: torch.Tensor, context: contexts.ContextDependency,
                alignment, semiring, lex_masks=None) -> tuple[torch.Tensor, torch.Tensor]:
  """(dist [B], alpha_0..T-1 [B, T, C]) over W [B, T, C, V+1]: alpha_0 = one
  at the start state; frames t >= num_frames[b] leave alpha unchanged; dist =
  (+) of the final alphas (every state is final, lattices.py:496).
  lex_masks: per expansion a tensor added to the lexical weights of that
  expansion (viterbi's derivative probes)."""
  K = expansions(alignment)
  B, T, C, _ = W.shape
  one = semiring.ones([], W.dtype)
  zero = semiring.zeros([], W.dtype)
  alpha = torch.where(torch.arange(C) == context.start(), one, zero).expand(B, C)
  alphas = []
  for t in range(T):
    alphas.append(alpha)
    blank, lex = W[:, t, :, 0], W[:, t, :, 1:]

    def step(x, i, lex=lex, t=t):
      li = lex if lex_masks is None else lex + lex_masks[i][:, t]
      return context.forward_reduce(semiring.times(x[..., None], li), semiring)

    nxt = _frame(alpha, step, blank, K, semiring)
    alpha = torch.where(_live(nf, t), nxt, alpha)
  alpha_all = torch.stack(alphas, dim=1) if alphas else W.new_zeros([B, 0, C])
  return semiring.sum(alpha, dim=-1), alpha_all


def string_weights(W: torch.Tensor, labels: torch.Tensor, context: contexts.ContextDependency):
  """Per frame the string lattice's arc weights [B, T, U+1]: blank[u] =
  W[ctx_u, 0] and lexical[u] = W[ctx_u, y_{u+1}] (the arc u -> u+1; none
  from u = U), ctx_u the context after the first u labels (walk_states,
  contexts.py:109-146). Labels outside 1..V read label 1's weight
  (make_safe_classes) and keep the context (epsilon)."""
  B, T, C, R = W.shape
  V = R - 1
  U = labels.shape[-1]
  lab = labels.long()
  ctx = context.walk_states(lab)                      # [B, U+1]
  safe = torch.where((lab >= 1) & (lab <= V), lab, torch.ones_like(lab))
  Wc = torch.gather(W, 2, ctx[:, None, :, None].expand(B, T, U + 1, R))  # [B, T, U+1, R]
  blank = Wc[..., 0]
  lex = torch.gather(Wc[:, :, :U, :], 3, safe[:, None, :, None].expand(B, T, U, 1))[..., 0]
  return blank, lex


def num_forward(W: torch.Tensor, nf: torch.Tensor, labels: torch.Tensor, nl: torch.Tensor,
                context: contexts.ContextDependency, alignment, semiring) -> torch.Tensor:
  """Shortest distance of the lattice intersected with the label string
  (lattices.py:250-377): alpha over string positions 0..U, read at nl. The
  lexical step on the string moves every position one place up."""
  blank, lex = string_weights(W, labels, context)
  return _string_distance(blank, lex, nf, nl, expansions(alignment), semiring)


def _string_distance(blank: torch.Tensor, lex: torch.Tensor, nf: torch.Tensor, nl: torch.Tensor,
                     K: int, semiring) -> torch.Tensor:
  """num_forward's recursion over the string's own weights (string_weights):
  blank [B, T, U+1], lex [B, T, U]."""
  W = blank
  B, T = blank.shape[:2]
  U = lex.shape[-1]
  dev = W.device  # the host, or the weights' own device (align_posteriors past its kernel's range)
  zero = semiring.zeros([B, 1], W.dtype, dev)
  one = semiring.ones([], W.dtype, dev)
  alpha = torch.where(torch.arange(U + 1, device=dev) == 0, one,
                      semiring.zeros([], W.dtype, dev)).expand(B, U + 1)
  for t in range(T):
    lex_t = torch.cat([lex[:, t], zero], dim=-1)   # no arc out of position U

    def step(x, i, lex_t=lex_t):
      return torch.cat([zero, semiring.times(x, lex_t)[:, :-1]], dim=-1)

    nxt = _frame(alpha, step, blank[:, t], K, semiring)
    alpha = torch.where(_live(nf, t), nxt, alpha)
  ok = (nl >= 0) & (nl <= U)
  num = torch.gather(alpha, 1, nl.clamp(0, U).long()[:, None])[:, 0]
  return torch.where(ok, num, semiring.zeros([], W.dtype, dev))


def loss(W: torch.Tensor, nf: torch.Tensor, labels: torch.Tensor, nl: torch.Tensor,
         context: contexts.ContextDependency, alignment, local_norm: bool) -> torch.Tensor:
  """-log P(labels | frames) = log_z - num, or -num for a locally
  normalised weight function (lattices.py:131-183)."""
  num = num_forward(W, nf, labels, nl, context, alignment, semirings.Log)
  if local_norm:
    out = -num
  else:
    log_z, _ = den_forward(W, nf, context, alignment, semirings.Log)
    out = log_z - num
  # an unreachable string (num = -inf, loss = +inf) contributes no gradient
  return torch.where(torch.isfinite(num), out, out.detach())


def viterbi(W: torch.Tensor, nf: torch.Tensor, context: contexts.ContextDependency, alignment,
            label_convention: str) -> tuple[torch.Tensor, torch.Tensor]:
  """Best path by differentiating the max-tropical distance w.r.t. zero
  lexical masks, one per expansion of a frame (lattices.py:185-247 has one,
  FrameDependent's only expansion): the one-hot derivative of mask i at
  frame t names the label of the frame's (i+1)-th lexical arc, all-zero
  means none. Returns labels [B, T * A] (A = 1 for FrameDependent, K + 1
  for FrameLabelDependent: slot i of a frame the (i+1)-th lexical label,
  else 0; the last slot is always 0) and the path weights. 'reference'
  emits label y as y - 1, 'true' emits y. Every utterance is
  decoded on its own (its distance depends on its own masks only)."""
  K = expansions(alignment)
  B, T, C, R = W.shape
  n_masks = max(K, 1)
  with torch.enable_grad():
    masks = [torch.zeros([B, T, 1, R - 1], dtype=W.dtype, requires_grad=True)
             for _ in range(n_masks)]
    dist, _ = den_forward(W.detach(), nf, context, alignment, semirings.MaxTropical,
                          lex_masks=masks)
    grads = torch.autograd.grad(dist.sum(), masks, allow_unused=True)
  slots = []
  for g in grads:
    g = torch.zeros([B, T, R - 1], dtype=W.dtype) if g is None else g[:, :, 0, :]
    blank = torch.all(g == 0, dim=-1)
    idx = torch.argmax(g, dim=-1)
    lexical = idx if label_convention == 'reference' else idx + 1
    slots.append(torch.where(blank, torch.zeros_like(idx), lexical))
  if K:
    slots.append(torch.zeros_like(slots[0]))
  return torch.stack(slots, dim=-1).reshape(B, T * len(slots)), dist.detach()


def align(W: torch.Tensor, nf: torch.Tensor, labels: torch.Tensor, nl: torch.Tensor,
          context: contexts.ContextDependency, alignment):
  """Forced alignment: the max-tropical string distance differentiated with
  respect to the string's own per-frame lexical weights (string_weights), in
  viterbi's style: the one-hot derivative at (t, u) says the arc leaving
  string position u is taken on frame t (first-argmax ties: the blank, then
  fewer expansions). Returns (alignment_labels [B, T * A], label_frames
  [B, U], path_weights [B]): slot i of frame t holds the true label (0 for an
  epsilon) of the frame's (i+1)-th lexical arc, else 0; label_frames is -1
  from num_labels on. Utterances of distance -inf are unaligned: all 0 / -1."""
  K = expansions(alignment)
  B, T = W.shape[:2]
  U = labels.shape[-1]
  V = W.shape[-1] - 1
  A = K + 1 if K else 1
  lab = labels.long()
  with torch.enable_grad():
    blank, lex = string_weights(W.detach(), lab, context)
    lex = lex.detach().requires_grad_(True)
    dist = _string_distance(blank, lex, nf, nl, K, semirings.MaxTropical)
    grad = (torch.autograd.grad(dist.sum(), [lex], allow_unused=True)[0]
            if dist.requires_grad else None)
  dist = dist.detach()
  taken = torch.zeros([B, T, U], dtype=torch.bool) if grad is None else grad > 0
  taken = taken & (dist > -torch.inf)[:, None, None]
  label_frames = torch.where(taken.any(dim=1), taken.int().argmax(dim=1),
                             torch.full([B, U], -1)).long()
  # the frame's lexical arcs are consecutive positions: their rank is the slot
  true = torch.where((lab >= 1) & (lab <= V), lab, torch.zeros_like(lab))
  slot = torch.cumsum(taken.long(), dim=2) - 1
  out = torch.zeros([B, T, A], dtype=torch.long)
  b, t, u = torch.nonzero(taken, as_tuple=True)
  out[b, t, slot[b, t, u]] = true[b, u]
  return out.reshape(B, T * A), label_frames, dist


def align_posteriors(W: torch.Tensor, nf: torch.Tensor, labels: torch.Tensor, nl: torch.Tensor,
                     context: contexts.ContextDependency, alignment):
  """Emission posteriors of the label string (include/lt_posterior.h): the
  Log string distance differentiated with respect to the string's own
  per-frame lexical weights (string_weights), align's construction in the Log
  semiring. emission[b, t, u] = d log_prob / d lex_t[u] is the posterior
  probability that the arc leaving string position u is taken on frame t
  (FrameLabelDependent: summed over the frame's expansion slots). Returns
  (emission [B, T, U], log_prob [B]), float32 (float64 for float64 weights). Rows t >= nf and
  columns u >= nl are exactly 0; an utterance whose distance is not finite is
  masked out of the differentiated sum: log_prob = -inf, emission all 0.
  Labels outside 1..V are epsilons. Runs on W's device (the host for CPU
  tensors; RecognitionLattice.align_posteriors runs it on a ROCm device past
  the kernel's range, with the context as a NextStateTable on that device)."""
  K = expansions(alignment)
  B, T = W.shape[:2]
  U = labels.shape[-1]
  V = W.shape[-1] - 1
  lab = labels.long()
  lab = torch.where((lab >= 1) & (lab <= V), lab, torch.zeros_like(lab))
  with torch.enable_grad():
    Wd = W.detach()
    if Wd.dtype != torch.float64:  # float64 stays (the tests' reference precision)
      Wd = Wd.float()
    blank, lex = string_weights(Wd, lab, context)
    lex = lex.detach().requires_grad_(True)
    dist = _string_distance(blank, lex, nf, nl, K, semirings.Log)
    fin = torch.isfinite(dist.detach())
    total = torch.where(fin, dist, torch.zeros_like(dist)).sum()
    grad = (torch.autograd.grad(total, [lex], allow_unused=True)[0]
            if total.requires_grad else None)
  dist = dist.detach()
  emission = torch.zeros([B, T, U], dtype=Wd.dtype, device=W.device)
  if grad is not None:
    emission = torch.where(fin[:, None, None], grad, emission)
  log_prob = torch.where(fin, dist, torch.full_like(dist, -torch.inf))
  return emission, log_prob


def align_expectation(W: torch.Tensor, nf: torch.Tensor, labels: torch.Tensor, nl: torch.Tensor,
                      context: contexts.ContextDependency, alignment,
                      lexical_values: torch.Tensor, blank_values: torch.Tensor):
  """(expected [B], log_prob [B]) of include/lt_string_expect.h: the posterior
  mean, over the alignments of the label string, of a path value given in
  string coordinates (lexical_values [B, T, U] for the arc leaving position u
  on frame t, blank_values [B, T, U+1] for the blank arc at position u).
  align_posteriors' construction kept in the graph: the Log string distance is
  differentiated with respect to the string's own lexical and blank weights
  (string_weights, with its graph to W) with create_graph, and expected is the
  sum of those derivatives (emission, blank_occ) times the values. So expected
  and log_prob are differentiable w.r.t. W, and expected w.r.t. the values, by
  ordinary autograd (d expected / dW is a second derivative of log_prob).
  FrameLabelDependent: the derivative sums a frame's expansion slots. Runs in
  W's dtype on W's device. Edge rules: a value where the derivative is 0 (an
  arc of weight -inf, rows t >= nf, columns past nl) is not read into the
  arithmetic; an utterance whose distance is not finite is masked out of the
  differentiated sum: log_prob = -inf, expected = 0, zero gradients."""
  K = expansions(alignment)
  B = W.shape[0]
  V = W.shape[-1] - 1
  lab = labels.long()
  lab = torch.where((lab >= 1) & (lab <= V), lab, torch.zeros_like(lab))
  wants_graph = torch.is_grad_enabled() and (W.requires_grad or lexical_values.requires_grad or
                                             blank_values.requires_grad)
  with torch.enable_grad():
    blank, lex = string_weights(W, lab, context)
    if not blank.requires_grad:
      blank, lex = blank.detach().requires_grad_(), lex.detach().requires_grad_()
    dist = _string_distance(blank, lex, nf, nl, K, semirings.Log)
    fin = torch.isfinite(dist.detach())
    total = torch.where(fin, dist, torch.zeros_like(dist)).sum()
    g_lex, g_blank = (torch.autograd.grad(total, [lex, blank], create_graph=True,
                                          allow_unused=True)
                      if total.requires_grad else (None, None))
    expected = torch.zeros([B], dtype=W.dtype, device=W.device)
    for g, val in ((g_lex, lexical_values), (g_blank, blank_values)):
      if g is None or g.numel() == 0:
        continue
      val = val.to(device=W.device, dtype=W.dtype)
      expected = expected + (g * torch.where(g.detach() != 0, val, torch.zeros_like(val))).sum(
          dim=(1, 2))
    expected = torch.where(fin, expected, torch.zeros_like(expected))
    log_prob = torch.where(fin, dist, torch.full_like(dist, -torch.inf).detach())
  if not wants_graph:
    expected, log_prob = expected.detach(), log_prob.detach()
  return expected, log_prob


def expectation(W: torch.Tensor, values: torch.Tensor, nf: torch.Tensor,
                context: contexts.ContextDependency) -> tuple[torch.Tensor, torch.Tensor]:
  """(E [B], log_z [B]) of include/lt_expect.h on the FrameDependent
  denominator lattice: E = sum_a m_a v_a with m = d log_z / dW taken with a
  graph, so E and log_z are differentiable w.r.t. W, and E w.r.t. values, by
  ordinary autograd (d E / dW is the second derivative of log_z). Runs in W's
  dtype. Edge rules: an arc with m = 0 (w = -inf, padding) contributes nothing
  and its value is not read into the arithmetic; an utterance whose log_z is
  not finite gives E = 0 and zero gradients, log_z as computed."""
  alignment = alignments.FrameDependent()
  wants_graph = torch.is_grad_enabled() and (W.requires_grad or values.requires_grad)
  with torch.no_grad():
    lz0, _ = den_forward(W, nf, context, alignment, semirings.Log)
  fin = torch.isfinite(lz0)
  with torch.enable_grad():
    # utterances without a finite log_z run on zero weights, detached from W
    Ws = torch.where(fin[:, None, None, None], W, torch.zeros_like(W))
    if not Ws.requires_grad:
      Ws = Ws.requires_grad_()
    log_z, _ = den_forward(Ws, nf, context, alignment, semirings.Log)
    (m,) = torch.autograd.grad(log_z.sum(), Ws, create_graph=True)
    v = torch.where(m > 0, values.to(W.dtype), torch.zeros_like(m))
    expected = (m * v).sum(dim=(1, 2, 3))
    expected = torch.where(fin, expected, torch.zeros_like(expected))
    log_z = torch.where(fin, log_z, lz0)
  if not wants_graph:
    expected, log_z = expected.detach(), log_z.detach()
  return expected, log_z


# ---------------------------------------------------------------------------
# Sampling paths from the lattice posterior (include/lt_sample.h)
# ---------------------------------------------------------------------------
_M32 = 0xffffffff


def _mulhilo(m: int, c: torch.Tensor):
  """(high, low) 32-bit words of m * c for int64 tensors holding 32-bit
  values: the high word from 16-bit halves of c (no product passes 2^49),
  the low word from the wrapping int64 product."""
  hi = (m * (c >> 16) + ((m * (c & 0xffff)) >> 16)) >> 16
  return hi, (m * c) & _M32


def philox4x32(counter, key):
  """Philox4x32-10 (Random123's constants and round function) on int64
  tensors of 32-bit words: counter = (c0, c1, c2, c3), key = (k0, k1), any
  broadcastable shapes. Returns the four output words."""
  c0, c1, c2, c3 = counter
  k0, k1 = key
  for _ in range(10):
    hi0, lo0 = _mulhilo(0xD2511F53, c0)
    hi1, lo1 = _mulhilo(0xCD9E8D57, c2)
    c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
    k0 = (k0 + 0x9E3779B9) & _M32
    k1 = (k1 + 0xBB67AE85) & _M32
  return c0, c1, c2, c3


def sample_noise(seed: int, b, s, t, k) -> torch.Tensor:
  """g(b, s, t, p, y) of include/lt_sample.h for k = p*(V+1) + y (int64
  tensors, broadcastable): -log(-log u), u = ((r >> 8) + 0.5) 2^-24, in fp32.
  u is an fp32 number while r >> 8 < 2^23; above that 1 - u is one, and
  -log u = -log1p(-(1 - u))."""
  k = torch.as_tensor(k)
  dev = k.device
  seed = int(seed) & 0xffffffffffffffff
  key = (torch.tensor(seed & _M32, device=dev), torch.tensor(seed >> 32, device=dev))
  shape = torch.broadcast_shapes(*(tuple(torch.as_tensor(x).shape) for x in (b, s, t, k)))
  ctr = [torch.as_tensor(x, device=dev).to(torch.int64).expand(shape) for x in (k >> 2, t, s, b)]
  out = philox4x32(ctr, key)
  sel = (k & 3).expand(shape)
  r = torch.where(sel < 2, torch.where(sel == 0, out[0], out[1]),
                  torch.where(sel == 2, out[2], out[3]))
  x = r >> 8
  low = -torch.log((x.float() + 0.5) * 2.0**-24)
  high = -torch.log1p(-(((1 << 25) - 2 * x - 1).float() * 2.0**-25))
  return -torch.log(torch.where(x < (1 << 23), low, high))


def _pick(score: torch.Tensor, k: torch.Tensor):
  """Index along the last dim of the largest score, ties to the smallest k;
  NaN scores never win (all NaN: the smallest k)."""
  score = torch.where(torch.isnan(score), torch.full_like(score, -torch.inf), score)
  best = score.max(dim=-1, keepdim=True).values
  big = torch.iinfo(torch.int64).max
  return torch.where(score == best, k, torch.full_like(k, big)).argmin(dim=-1)


def _in_arc_table(table: torch.Tensor):
  """The arcs into each state, padded: (k [C, D], p [C, D], valid [C, D]),
  candidate 0 the blank arc (q, 0), then the in-arcs (p, y) with
  table[p, y-1] = q; k = p*(V+1) + y."""
  C, V = table.shape
  dst = table.reshape(-1).long()
  order = torch.argsort(dst, stable=True)
  deg = torch.bincount(dst, minlength=C)
  D = int(deg.max()) + 1
  start = torch.cumsum(deg, 0) - deg
  rank = torch.arange(C * V, device=table.device) - start[dst[order]]
  p = order // V
  k = p * (V + 1) + order % V + 1
  q = torch.arange(C, device=table.device)
  ck = torch.zeros([C, D], dtype=torch.int64, device=table.device)
  cp = torch.zeros_like(ck)
  ok = torch.zeros([C, D], dtype=torch.bool, device=table.device)
  ck[:, 0], cp[:, 0], ok[:, 0] = q * (V + 1), q, True
  ck[dst[order], rank + 1] = k
  cp[dst[order], rank + 1] = p
  ok[dst[order], rank + 1] = True
  return ck, cp, ok


def sample(W: torch.Tensor, nf: torch.Tensor, context: contexts.ContextDependency,
           num_samples: int, seed: int, log_z: torch.Tensor = None, alpha: torch.Tensor = None):
  """num_samples paths per utterance from p(pi) = exp(w(pi)) / Z of the
  denominator lattice x FrameDependent, by the definition of
  include/lt_sample.h (Gumbel-max on Philox4x32-10, walked backwards over
  alpha) in torch ops: one step per frame, vectorised over utterances,
  samples and candidate arcs. Device-agnostic when log_z [B] and alpha
  [B, T, C] (the Log forward's) are given; else they come from den_forward.
  Returns (labels int64 [B, S, T], path weights [B, S], log_z [B])."""
  if not hasattr(context, 'next_state_table'):
    raise NotImplementedError(f'{type(context).__name__} has no next-state table')
  table = context.next_state_table
  table = torch.as_tensor(table() if callable(table) else table).to(W.device)
  if log_z is None or alpha is None:
    log_z, alpha = den_forward(W, nf, context, alignments.FrameDependent(), semirings.Log)
  W = W.float()
  alpha = alpha.float()
  dev = W.device
  B, T, C, R = W.shape
  S = int(num_samples)
  nf = nf.to(dev).long().clamp(0, T)
  nf_host = nf.tolist()
  sampled = torch.isfinite(log_z.to(dev))
  ck, cp, ok = _in_arc_table(table)
  bb = torch.arange(B, device=dev)[:, None, None]
  ss = torch.arange(S, device=dev)[None, :, None]
  all_k = torch.arange(C * R, device=dev)
  labels = torch.zeros([B, S, T], dtype=torch.int64, device=dev)
  weight = torch.zeros([B, S], dtype=torch.float32, device=dev)
  q = torch.zeros([B, S], dtype=torch.int64, device=dev)
  neg = torch.tensor(-torch.inf, device=dev)
  for t in range(max(nf_host, default=0) - 1, -1, -1):
    Wt = W[:, t].reshape(B, C * R)
    # the arcs into q (frames before the last live one)
    k, p, valid = ck[q], cp[q], ok[q]                               # [B, S, D]
    a = torch.gather(alpha[:, t], 1, p.reshape(B, -1)).reshape(p.shape)
    w = torch.gather(Wt, 1, k.reshape(B, -1)).reshape(k.shape)
    score = torch.where(valid, (a + w) + sample_noise(seed, bb, ss, t, k), neg)
    j = _pick(score, torch.where(valid, k, torch.full_like(k, C * R)))[..., None]
    kw, pw, ww = (torch.gather(x, 2, j)[..., 0] for x in (k, p, w))
    last = [b for b in range(B) if nf_host[b] - 1 == t]
    if last:  # the last live frame: every arc of the frame
      lb = torch.tensor(last, device=dev)
      kk = all_k.expand(len(last), S, C * R)
      al = alpha[lb, t][:, None, all_k // R]
      wl = Wt[lb][:, None, :].expand(len(last), S, C * R)
      sc = (al + wl) + sample_noise(seed, lb[:, None, None], ss, t, kk)
      jl = _pick(sc, kk)
      kw[lb], pw[lb], ww[lb] = jl, jl // R, torch.gather(wl, 2, jl[..., None])[..., 0]
    live = (t < nf)[:, None]
    labels[:, :, t] = torch.where(live, kw - pw * R, labels[:, :, t])
    weight = torch.where(live, weight + ww, weight)
    q = torch.where(live, pw, q)
  labels = torch.where(sampled[:, None, None], labels, torch.zeros_like(labels))
  weight = torch.where(sampled[:, None], weight, neg)
  return labels, weight, log_z


# ---------------------------------------------------------------------------
# Scoring given paths and the edit distance of hypotheses (include/lt_paths.h)
# ---------------------------------------------------------------------------
def path_weights(W: torch.Tensor, nf: torch.Tensor, labels: torch.Tensor,
                 context: contexts.ContextDependency):
  """(path weights [B, S], states int32 [B, S, T]) of the paths labels
  [B, S, T] (the true label per frame, 0 = blank) through W [B, T, C, V+1], by
  the definition of include/lt_paths.h in torch ops: the walk of the
  next-state table from state 0 (one step per frame, vectorised over
  utterances and paths), one gather, and the fp32 sum taken from the last
  frame to the first, the order of `sample`. A live label outside [0, V]
  gives weight -inf and states -1. Differentiable w.r.t. W by plain autograd;
  device-agnostic."""
  if not hasattr(context, 'next_state_table'):
    raise NotImplementedError(f'{type(context).__name__} has no next-state table')
  table = context.next_state_table
  table = torch.as_tensor(table() if callable(table) else table).to(W.device).long()
  dev = W.device
  B, T, C, R = W.shape
  V = R - 1
  labels = labels.to(dev).long()
  if labels.ndim != 3 or labels.shape[0] != B or labels.shape[2] != T:
    raise ValueError(f'alignment labels {tuple(labels.shape)} do not match [{B}, S, {T}]')
  S = labels.shape[1]
  nf = nf.to(dev).long().clamp(0, T)
  live = torch.arange(T, device=dev)[None, None, :] < nf[:, None, None]      # [B, 1, T]
  inside = (labels >= 0) & (labels <= V)
  valid = (inside | ~live).all(dim=-1)                                        # [B, S]
  lex = live & (labels >= 1) & (labels <= V)
  q = torch.zeros([B, S], dtype=torch.int64, device=dev)
  states = []
  for t in range(T):
    states.append(q)
    y = labels[:, :, t]
    q = torch.where(lex[:, :, t], table[q, (y - 1).clamp(0, V - 1)], q)
  states = torch.stack(states, dim=2) if states else q.new_zeros([B, S, 0])
  on = live & valid[:, :, None]                                               # [B, S, T]
  k = states * R + labels.clamp(0, V)
  w = torch.gather(W.float().reshape(B, T, C * R), 2, k.permute(0, 2, 1)).permute(0, 2, 1)
  w = torch.where(on, w, torch.zeros_like(w))
  total = torch.zeros([B, S], dtype=torch.float32, device=dev)
  for t in range(T - 1, -1, -1):
    total = total + w[:, :, t]
  total = torch.where(valid, total, torch.full_like(total, -torch.inf))
  states = torch.where(on, states, torch.full_like(states, -1)).to(torch.int32)
  return total, states


def edit_distance(hyp: torch.Tensor, nf, ref: torch.Tensor, nl: torch.Tensor):
  """(distance int32 [B, S], hypothesis token counts int32 [B, S]) by the
  definition of include/lt_paths.h in torch ops: the tokens (values > 0) of
  hyp [B, S, T] below nf [B] (None: all T) against those of ref [B, U] below
  nl [B], unit-cost Levenshtein; nl outside [0, U] gives -1. One DP row
  update per hypothesis token, vectorised over utterances, hypotheses and
  reference positions, with the insertion chain as a cumulative minimum.
  Device-agnostic."""
  dev = hyp.device
  hyp = hyp.long()
  B, S, T = hyp.shape
  ref = ref.to(dev).long().reshape(B, -1)
  U = ref.shape[1]
  nl = nl.to(dev).long()
  ranged = (nl >= 0) & (nl <= U)
  nfc = torch.full([B], T, device=dev) if nf is None else nf.to(dev).long().clamp(0, T)
  hok = (hyp > 0) & (torch.arange(T, device=dev)[None, None, :] < nfc[:, None, None])
  rok = (ref > 0) & (torch.arange(U, device=dev)[None, :] < nl[:, None])
  # tokens first, in their order
  hyp_c = torch.gather(hyp, 2, torch.argsort((~hok).long(), dim=2, stable=True))
  ref_c = torch.gather(ref, 1, torch.argsort((~rok).long(), dim=1, stable=True))
  hlen = hok.sum(dim=2)                                                       # [B, S]
  n = rok.sum(dim=1)                                                          # [B]
  j = torch.arange(U + 1, device=dev)
  D = j.expand(B, S, U + 1)
  big = torch.full([B, S, 1], T + U + 2, device=dev)
  for i in range(int(hlen.max()) if hlen.numel() else 0):
    h = hyp_c[:, :, i]
    sub = D[:, :, :-1] + (ref_c[:, None, :] != h[:, :, None]).long()
    tmp = torch.minimum(D + 1, torch.cat([big, sub], dim=2))
    new = j + torch.cummin(tmp - j, dim=2).values
    D = torch.where((i < hlen)[:, :, None], new, D)
  dist = torch.gather(D, 2, n[:, None, None].expand(B, S, 1))[..., 0]
  dist = torch.where(ranged[:, None], dist, torch.full_like(dist, -1))
  return dist.to(torch.int32), hlen.to(torch.int32)


# ---------------------------------------------------------------------------
# Prefix beam search: the N best label sequences (include/lt_beam.h)
# ---------------------------------------------------------------------------
_M64 = (1 << 64) - 1


def _i64(x: int) -> int:
  """The int64 that holds the bits of the unsigned 64-bit x."""
  x &= _M64
  return x - (1 << 64) if x >> 63 else x


def _lsr(z: torch.Tensor, k: int) -> torch.Tensor:
  """Logical shift right of int64 bit patterns."""
  return (z >> k) & ((1 << (64 - k)) - 1)


def prefix_hash(h: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
  """mix(h, y) of include/lt_beam.h on int64 tensors holding unsigned 64-bit
  patterns (int64 products wrap, shifts are made logical)."""
  z = h ^ (y * _i64(0x9E3779B97F4A7C15))
  z = (z ^ _lsr(z, 30)) * _i64(0xBF58476D1CE4E5B9)
  z = (z ^ _lsr(z, 27)) * _i64(0x94D049BB133111EB)
  return z ^ _lsr(z, 31)


def beam_search(W: torch.Tensor, nf: torch.Tensor, context: contexts.ContextDependency,
                beam_size: int, semiring, want_trace: bool = False):
  """The beam_size best label sequences per utterance of the denominator
  lattice x FrameDependent, by the definition of include/lt_beam.h in torch
  ops, fp32: one step per frame, vectorised over utterances, slots and labels
  (candidates, the merge of a prefix with its parent's extension, a stable
  descending sort for the selection), then the backtrace of the trace.
  Device-agnostic. Returns (labels int64 [B, K, T], num_labels int64 [B, K],
  scores fp32 [B, K]) and, with want_trace, (trace int32 [B, T, K], step_score
  fp32 [B, T, K])."""
  if not hasattr(context, 'next_state_table'):
    raise NotImplementedError(f'{type(context).__name__} has no next-state table')
  name = getattr(semiring, 'name', None)
  if name not in ('Log', 'MaxTropical'):
    raise NotImplementedError(f'beam_search supports Log and MaxTropical, got {semiring!r}')
  K = int(beam_size)
  if K < 1:
    raise ValueError(f'beam_size should be >= 1, but got {beam_size}')
  table = context.next_state_table
  table = torch.as_tensor(table() if callable(table) else table).to(W.device).long()
  W = W.float()
  dev = W.device
  B, T, C, R = W.shape
  nf = nf.to(dev).long().clamp(0, T)
  neg = torch.tensor(-torch.inf, device=dev)
  s = torch.full([B, K], -torch.inf, device=dev)
  s[:, 0] = 0.
  c = torch.zeros([B, K], dtype=torch.int64, device=dev)
  n, h, ph, y = (torch.zeros_like(c) for _ in range(4))
  trace = torch.full([B, T, K], -1, dtype=torch.int32, device=dev)
  step = torch.full([B, T, K], -torch.inf, device=dev)
  last = int(nf.max()) if B else 0
  for t in range(last):
    rows = torch.gather(W[:, t], 1, c[:, :, None].expand(B, K, R))             # [B, K, R]
    cand = s[:, :, None] + rows
    cand = torch.where(torch.isnan(cand), neg, cand)
    alive = s > -torch.inf
    # merge: slot i's parent j, whose extension by y_i is slot i's prefix
    match = (alive[:, :, None] & alive[:, None, :] & (n[:, :, None] >= 1) &
             (h[:, None, :] == ph[:, :, None]) & (n[:, None, :] == n[:, :, None] - 1))
    has = match.any(dim=2)
    j = match.to(torch.int8).argmax(dim=2)                                    # the lowest
    flat = cand.reshape(B, K * R)
    at = j * R + y
    ext = torch.gather(flat, 1, at)
    blank = cand[:, :, 0]
    if name == 'Log':
      both = torch.logaddexp(blank, ext)
      both = torch.where((blank == -torch.inf) & (ext == -torch.inf), neg, both)
    else:
      both = torch.where(blank >= ext, blank, ext)
    both = torch.where(torch.isnan(both), neg, both)
    gone = torch.zeros([B, K * R + 1], dtype=torch.bool, device=dev)
    gone.scatter_(1, torch.where(has, at, torch.full_like(at, K * R)), True)
    flat = torch.where(gone[:, :K * R], neg, flat).reshape(B, K, R).clone()
    flat[:, :, 0] = torch.where(has, both, blank)
    # select: larger score first, equal scores to the smaller k (stable sort)
    val, k = torch.sort(flat.reshape(B, K * R), dim=1, descending=True, stable=True)
    val, k = val[:, :K], k[:, :K]
    kept = val > -torch.inf
    src, yw = k // R, k % R
    g = lambda x: torch.gather(x, 1, src)
    ext_sel = yw > 0
    hs = g(h)
    new = dict(
        s=torch.where(kept, val, neg),
        c=torch.where(ext_sel, table[g(c), (yw - 1).clamp(min=0)], g(c)),
        n=g(n) + ext_sel.long(),
        h=torch.where(ext_sel, prefix_hash(hs, yw), hs),
        ph=torch.where(ext_sel, hs, g(ph)),
        y=torch.where(ext_sel, yw, g(y)))
    zero = torch.zeros_like(c)
    for key in ('c', 'n', 'h', 'ph', 'y'):
      new[key] = torch.where(kept, new[key], zero)
    live = (t < nf)[:, None]
    s, c, n = torch.where(live, new['s'], s), torch.where(live, new['c'], c), torch.where(live, new['n'], n)
    h, ph, y = torch.where(live, new['h'], h), torch.where(live, new['ph'], ph), torch.where(live, new['y'], y)
    trace[:, t] = torch.where(live & kept, (src << 16) | yw, torch.full_like(src, -1)).to(torch.int32)
    step[:, t] = torch.where(live & kept, val, neg)
  # backtrace: each final slot's labels, back to front
  labels = torch.zeros([B, K, T + 1], dtype=torch.int64, device=dev)   # column T: scratch
  cur = torch.arange(K, device=dev).expand(B, K)
  pos = n.clone()
  for t in range(last - 1, -1, -1):
    e = torch.gather(trace[:, t].long(), 1, cur)
    on = (t < nf)[:, None] & (s > -torch.inf) & (e >= 0)
    yy = e & 0xffff
    put = on & (yy > 0) & (pos > 0)
    pos = pos - put.long()
    labels.scatter_(2, torch.where(put, pos, torch.full_like(pos, T))[:, :, None],
                    torch.where(put, yy, torch.zeros_like(yy))[:, :, None])
    cur = torch.where(on, e >> 16, cur)
  out = (labels[:, :, :T].contiguous(), n, s)
  return out + (trace, step) if want_trace else out
