"""PyTorch CPU path of the lattice algorithms, for CPU tensors.

``RecognitionLattice`` runs here when its arc weights live on the CPU and on
the HIP kernels (liblt_lattice.so) when they live on a ROCm device: the
device of the tensors picks the implementation, as in the reference, and
there is no fallback from one to the other (a ROCm tensor never runs here;
a missing HIP library raises).

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
  zero = semiring.zeros([B, 1], W.dtype)
  one = semiring.ones([], W.dtype)
  alpha = torch.where(torch.arange(U + 1) == 0, one, semiring.zeros([], W.dtype)).expand(B, U + 1)
  for t in range(T):
    lex_t = torch.cat([lex[:, t], zero], dim=-1)   # no arc out of position U

    def step(x, i, lex_t=lex_t):
      return torch.cat([zero, semiring.times(x, lex_t)[:, :-1]], dim=-1)

    nxt = _frame(alpha, step, blank[:, t], K, semiring)
    alpha = torch.where(_live(nf, t), nxt, alpha)
  ok = (nl >= 0) & (nl <= U)
  num = torch.gather(alpha, 1, nl.clamp(0, U).long()[:, None])[:, 0]
  return torch.where(ok, num, semiring.zeros([], W.dtype))


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
