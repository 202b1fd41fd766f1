"""Float64 / NumPy reference of prefix beam search (include/lt_beam.h) -- TEST
INFRASTRUCTURE. Prefixes are tuples of labels and are compared as tuples: no
hashes here, so a wrong hash, a missed merge or a merge of different prefixes
in an implementation shows.

  search   the definition itself, one utterance at a time.
  replay   checks an implementation's trace / step_score frame by frame. The
           beam before frame t is the implementation's own (its prefixes
           rebuilt from the trace, its scores as given), so fp32 rounding and
           near-ties do not accumulate: every frame is judged on its own.
  backtrace  the label sequence of a final slot, walked back through the trace.
"""
import numpy as np


def bound(x):
  """The project's alpha parity bound (test_gpu_sample.py)."""
  return 1e-4 + 1e-4 * abs(x)


def make_weights(rng, B, T, C, V, bias):
  """N(0, 1) weights with a blank bias: with it a beam holds prefixes together
  with their parents, so merging matters (3 at V = 32, 1.5 at V <= 6)."""
  W = rng.standard_normal([B, T, C, V + 1]).astype(np.float32)
  W[..., 0] += np.float32(bias)
  return W


def _plus(a, b, semiring):
  if semiring == 'MaxTropical':
    return max(a, b)
  if a == -np.inf and b == -np.inf:
    return -np.inf
  return float(np.logaddexp(a, b))


def context_of(prefix, table):
  c = 0
  for y in prefix:
    c = int(table[c, y - 1])
  return c


def candidates(slots, Wt, table, semiring):
  """{(i, y): score} of one frame after the merge, from slots = [(prefix,
  score)] (all live) and the frame's W [C, V+1]; NaN sums count as -inf."""
  R = Wt.shape[1]
  cand = {}
  for i, (p, s) in enumerate(slots):
    row = Wt[context_of(p, table)].astype(np.float64)
    for y in range(R):
      v = s + row[y]
      cand[(i, y)] = -np.inf if np.isnan(v) else float(v)
  where = {p: i for i, (p, _) in enumerate(slots)}
  for i, (p, _) in enumerate(slots):
    if p and p[:-1] in where:
      j = where[p[:-1]]
      cand[(i, 0)] = _plus(cand[(i, 0)], cand.pop((j, p[-1])), semiring)
  return cand


def search(W, nf, table, K, semiring):
  """Per utterance the final beam [(prefix, score)], best first."""
  W = np.asarray(W)
  R = W.shape[3]
  out = []
  for b in range(W.shape[0]):
    slots = [((), 0.0)]
    for t in range(int(nf[b])):
      cand = candidates(slots, W[b, t], table, semiring)
      order = sorted((k for k, v in cand.items() if v > -np.inf),
                     key=lambda k: (-cand[k], k[0] * R + k[1]))[:K]
      slots = [(slots[i][0] + ((y,) if y else ()), cand[(i, y)]) for i, y in order]
    out.append(slots)
  return out


def replay(W, nf, table, K, semiring, trace, step_score):
  """Asserts (a)-(e) of the module docstring's contract on every live frame:
    (a) a kept slot's step_score is within bound of its recomputed candidate;
    (b) no discarded finite candidate exceeds the smallest kept recomputed
        score by more than 2 bound;
    (c) kept scores are non-increasing within bound;
    (d) no two kept slots hold the same prefix;
    (e) the number of live slots is min(K, finite candidates), and they are
        slots 0..m-1;
  and that padding frames are -1 / -inf. Returns (steps, final) with final[b]
  = [(prefix, score)] of the live slots after the last live frame."""
  W = np.asarray(W)
  B, T = W.shape[:2]
  trace = np.asarray(trace)
  step_score = np.asarray(step_score, np.float64)
  assert trace.shape == (B, T, K) and step_score.shape == (B, T, K)
  steps, final = 0, []
  for b in range(B):
    slots = [((), 0.0)]
    for t in range(int(nf[b])):
      cand = candidates(slots, W[b, t], table, semiring)
      finite = {k: v for k, v in cand.items() if v > -np.inf}
      tr, sc = trace[b, t], step_score[b, t]
      m = int((tr >= 0).sum())
      assert (tr[:m] >= 0).all() and (tr[m:] == -1).all(), (b, t, tr)
      assert (sc[m:] == -np.inf).all(), (b, t, sc)
      assert m == min(K, len(finite)), (b, t, m, len(finite))                    # (e)
      kept = [(int(e) >> 16, int(e) & 0xffff) for e in tr[:m]]
      assert len(set(kept)) == m, (b, t, kept)
      new = []
      for r, (i, y) in enumerate(kept):
        assert (i, y) in finite, (b, t, r, i, y, 'not a finite candidate (removed, dead or -inf)')
        assert abs(sc[r] - finite[(i, y)]) <= bound(finite[(i, y)]), (b, t, r, sc[r],   # (a)
                                                                      finite[(i, y)])
        if r:
          assert sc[r] <= sc[r - 1] + bound(sc[r - 1]), (b, t, r, sc[r - 1], sc[r])     # (c)
        new.append((slots[i][0] + ((y,) if y else ()), float(sc[r])))
      if m:
        low = min(finite[k] for k in kept)
        rest = [v for k, v in finite.items() if k not in set(kept)]
        if rest:
          assert max(rest) <= low + 2 * bound(low), (b, t, max(rest), low)              # (b)
      assert len({p for p, _ in new}) == m, (b, t, 'two slots hold one prefix')         # (d)
      slots = new
      steps += 1
    assert (trace[b, int(nf[b]):] == -1).all() and (step_score[b, int(nf[b]):] == -np.inf).all()
    final.append(slots)
  return steps, final


def backtrace(trace_b, nf_b, r):
  """The labels of final slot r of one utterance, walked back through its
  trace [T, K] from frame nf_b - 1."""
  out, cur = [], r
  for t in range(int(nf_b) - 1, -1, -1):
    e = int(trace_b[t, cur])
    assert e >= 0
    if e & 0xffff:
      out.append(e & 0xffff)
    cur = e >> 16
  return tuple(reversed(out))


def check_outputs(final, trace, nf, labels, num_labels, scores):
  """The final outputs against the replayed last live frame and the NumPy
  backtrace: labels packed at the front with zeros behind, lengths, scores bit
  for bit those of the last step_score row; dead slots all 0 / 0 / -inf."""
  labels, num_labels, scores = np.asarray(labels), np.asarray(num_labels), np.asarray(scores)
  B, K, T = labels.shape
  for b in range(B):
    m = len(final[b])
    for r in range(K):
      if r < m:
        p = final[b][r][0]
        if nf[b] > 0:
          assert backtrace(trace[b], nf[b], r) == p
          assert scores[b, r] == np.float32(final[b][r][1])
        else:
          assert p == () and scores[b, r] == 0
        assert num_labels[b, r] == len(p), (b, r)
        assert tuple(labels[b, r, :len(p)]) == p and not labels[b, r, len(p):].any(), (b, r)
      else:
        assert not labels[b, r].any() and num_labels[b, r] == 0 and scores[b, r] == -np.inf
