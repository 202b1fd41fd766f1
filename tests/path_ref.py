"""NumPy restatement of include/lt_paths.h, shared by tests/test_paths_cpu.py,
tests/test_gpu_paths.py, tests/test_gpu_edit_distance.py and
tests/test_gpu_sampled_risk.py -- TEST INFRASTRUCTURE.

  score     the walk of the next-state table from state 0 (Python ints), the
            path weight as a float64 sum and, separately, as the fp32 sum the
            header fixes: np.float32 adds from the last live frame to the
            first, started at 0.
  scatter   the dense float64 dW of one scalar per path by np.add.at.
  edit_distance   a plain two-row Levenshtein over the tokens (values > 0).
"""
import numpy as np


def score(W, nf, table, labels):
  """(weight32 fp32 [B, S], weight64 float64 [B, S], magnitude float64 [B, S],
  states int32 [B, S, T]) of labels [B, S, T] through W [B, T, C, V+1]:
  weight32 in the header's summation order, weight64 / magnitude the float64
  sums of w and |w| along the path. Invalid paths (a live label outside
  [0, V]): weight -inf, magnitude 0, states -1."""
  W = np.asarray(W)
  W32 = W.astype(np.float32)
  labels = np.asarray(labels)
  B, S, T = labels.shape
  V = table.shape[1]
  w32 = np.zeros([B, S], np.float32)
  w64 = np.zeros([B, S], np.float64)
  mag = np.zeros([B, S], np.float64)
  states = np.full([B, S, T], -1, np.int32)
  for b in range(B):
    n = min(max(int(nf[b]), 0), T)
    for s in range(S):
      ys = [int(y) for y in labels[b, s, :n]]
      if any(y < 0 or y > V for y in ys):
        w32[b, s] = w64[b, s] = -np.inf
        continue
      q, qs = 0, []
      for y in ys:
        qs.append(q)
        if y:
          q = int(table[q, y - 1])
      states[b, s, :n] = qs
      acc = np.float32(0)
      with np.errstate(invalid='ignore', over='ignore'):
        for t in range(n - 1, -1, -1):
          acc = np.float32(acc + W32[b, t, qs[t], ys[t]])
      w32[b, s] = acc
      arcs = np.array([float(W32[b, t, qs[t], ys[t]]) for t in range(n)], np.float64)
      w64[b, s] = arcs.sum()
      mag[b, s] = np.abs(arcs).sum()
  return w32, w64, mag, states


def scatter(shape, nf, labels, states, grad):
  """(dW float64 `shape` = [B, T, C, V+1], |grad| scattered the same way):
  dW[b,t,q,y] = sum_s grad[b,s] 1[states[b,s,t] = q, labels[b,s,t] = y]."""
  labels = np.asarray(labels)
  states = np.asarray(states)
  B, S, T = labels.shape
  dW = np.zeros(shape, np.float64)
  mag = np.zeros(shape, np.float64)
  live = (np.arange(T)[None, None, :] < np.clip(np.asarray(nf), 0, T)[:, None, None])
  on = live & (states >= 0)
  b, s, t = np.nonzero(on)
  g = np.asarray(grad, np.float64)[b, s]
  idx = (b, t, states[b, s, t], labels[b, s, t])
  np.add.at(dW, idx, g)
  np.add.at(mag, idx, np.abs(g))
  return dW, mag


def levenshtein(a, b):
  """Unit-cost edit distance of two token lists, two rows."""
  prev = list(range(len(b) + 1))
  for i, x in enumerate(a, 1):
    cur = [i]
    for j, y in enumerate(b, 1):
      cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
    prev = cur
  return prev[len(b)]


def edit_distance(hyp, nf, ref, nl):
  """(distance int32 [B, S], hyp_length int32 [B, S]) by the header's
  definition; nf None means every position of hyp counts."""
  hyp = np.asarray(hyp)
  ref = np.asarray(ref)
  B, S, T = hyp.shape
  U = ref.shape[1]
  dist = np.zeros([B, S], np.int32)
  length = np.zeros([B, S], np.int32)
  for b in range(B):
    n = T if nf is None else min(max(int(nf[b]), 0), T)
    ranged = 0 <= int(nl[b]) <= U
    r = [int(x) for x in ref[b, :int(nl[b])] if x > 0] if ranged else []
    for s in range(S):
      h = [int(x) for x in hyp[b, s, :n] if x > 0]
      length[b, s] = len(h)
      dist[b, s] = levenshtein(h, r) if ranged else -1
  return dist, length
