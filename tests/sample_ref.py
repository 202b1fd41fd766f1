"""Float64 NumPy restatement of the path sampler's definition
(include/lt_sample.h), shared by tests/test_sample_cpu.py and
tests/test_gpu_sample.py: an independent Philox4x32-10, the noise, the Log
forward, path enumeration, the forward walk of a label sequence and the
step-by-step replay of a sampled path."""
import itertools

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xffffffff)

# Random123's known answers: (counter words, key words, output words)
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox(counter, key):
  """Philox4x32-10 on uint64 arrays of 32-bit words (a 32 x 32 bit product
  fits 64 bits)."""
  c = [np.asarray(x, dtype=np.uint64) for x in counter]
  k0, k1 = int(key[0]), int(key[1])
  for _ in range(10):
    p0, p1 = M0 * c[0], M1 * c[2]
    c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK,
         (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
    k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
  return c


def noise(seed, b, s, t, k):
  """g(b, s, t, p, y) in float64 for an array of arcs k = p*(V+1) + y."""
  k = np.asarray(k, dtype=np.uint64)
  z = np.zeros_like(k)
  out = philox((k >> np.uint64(2), z + np.uint64(t), z + np.uint64(s), z + np.uint64(b)),
               (seed & 0xffffffff, seed >> 32))
  r = np.choose((k & np.uint64(3)).astype(np.int64), out)
  u = ((r >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0**-24
  return -np.log(-np.log(u))


def forward(W, nf, table):
  """(log_z [B], alpha [B, T, C]) of the denominator lattice in float64:
  alpha_t before frame t, start state 0, every state final."""
  W = np.asarray(W, np.float64)
  B, T, C, R = W.shape
  dst = np.asarray(table).reshape(-1)
  alpha = np.full([B, T, C], -np.inf)
  log_z = np.zeros([B])
  with np.errstate(invalid='ignore', divide='ignore'):
    for b in range(B):
      a = np.full([C], -np.inf)
      a[0] = 0.0
      for t in range(T):
        alpha[b, t] = a
        if t < nf[b]:
          new = a + W[b, t, :, 0]
          np.logaddexp.at(new, dst, (a[:, None] + W[b, t, :, 1:]).reshape(-1))
          a = new
      m = a.max()
      log_z[b] = m + np.log(np.exp(a - m).sum()) if np.isfinite(m) else m
  return log_z, alpha


def walk(labels, table):
  """States before each frame of a label sequence, from state 0."""
  q, states = 0, []
  for y in labels:
    states.append(q)
    if y:
      q = int(table[q, y - 1])
  return states


def path_weight(W, labels, table):
  """(float64 sum of the arc weights along labels, sum of their magnitudes)."""
  w = np.array([float(W[t, q, y]) for t, (q, y) in enumerate(zip(walk(labels, table), labels))])
  return w.sum(), np.abs(w).sum()


def path_probabilities(W, table, T):
  """{labels: p} over every label sequence of T frames of one utterance."""
  V = table.shape[1]
  seqs = list(itertools.product(range(V + 1), repeat=T))
  w = np.array([path_weight(W, s, table)[0] for s in seqs])
  p = np.exp(w - w.max())
  return dict(zip(seqs, p / p.sum()))


def count_units(counts, probs, S):
  """max over outcomes of |count - S p| / (sqrt(S p (1 - p)) + 1)."""
  p = np.asarray(probs, np.float64)
  return float(np.max(np.abs(np.asarray(counts) - S * p) / (np.sqrt(S * p * (1 - p)) + 1)))


def in_arcs(table):
  """Per state the arcs into it as arrays (k, p): the blank arc, then the
  in-arcs of the table."""
  C, V = table.shape
  R = V + 1
  cand = [([q * R], [q]) for q in range(C)]
  for p in range(C):
    for y in range(1, R):
      ks, ps = cand[int(table[p, y - 1])]
      ks.append(p * R + y)
      ps.append(p)
  return [(np.array(k), np.array(p)) for k, p in cand]


def replay(W, nf, table, labels, seed, alpha, rtol=1e-4, atol=1e-4):
  """Follows every sampled path (labels [B, S, T]) backwards and recomputes
  each step's candidate scores in float64 (alpha [B, T, C] float64): the pick
  must score at least best - 2 (atol + rtol |best|), the alpha bound once for
  each of the two scores compared. Returns (steps checked, worst shortfall in
  units of that bound)."""
  W = np.asarray(W, np.float64)
  B, S, T = labels.shape
  C, R = W.shape[2:]
  cand = in_arcs(table)
  all_k = np.arange(C * R)
  steps, worst = 0, 0.0
  for b in range(B):
    for s in range(S):
      states = walk(labels[b, s, :nf[b]], table)
      for t in range(nf[b] - 1, -1, -1):
        p, y = states[t], int(labels[b, s, t])
        if t == nf[b] - 1:
          ks, ps = all_k, all_k // R
        else:
          ks, ps = cand[states[t + 1]]
        with np.errstate(invalid='ignore'):
          score = alpha[b, t, ps] + W[b, t].reshape(-1)[ks] + noise(seed, b, s, t, ks)
        pick = np.nonzero(ks == p * R + y)[0]
        assert pick.size == 1, f'(b={b}, s={s}, t={t}): arc ({p}, {y}) is no candidate'
        best = np.nanmax(score)
        bound = 2 * (atol + rtol * abs(best))
        short = (best - score[pick[0]]) / bound
        assert short <= 1, (f'(b={b}, s={s}, t={t}): picked arc ({p}, {y}) scores '
                            f'{score[pick[0]]}, best {best}')
        worst = max(worst, short)
        steps += 1
  return steps, worst


# ---------------------------------------------------------------------------
# Checks both test files run, on CPU tensors and on the GPU
# ---------------------------------------------------------------------------
def table_of(context):
  t = context.next_state_table
  return (t() if callable(t) else t).numpy()


def random_table(rng, C, V):
  import torch
  return torch.tensor(rng.integers(0, C, [C, V]).astype(np.int32))


def _bigram_v2(rng):
  import last_torch_amd as lt
  return lt.contexts.FullNGram(vocab_size=2, context_size=1)


def _table_c4_v3(rng):
  import last_torch_amd as lt
  return lt.contexts.NextStateTable(random_table(rng, 4, 3))


# name: (context factory, T, number of paths)
DISTRIBUTIONS = {'bigram_v2_t4': (_bigram_v2, 4, 81), 'table_c4_v3_t3': (_table_c4_v3, 3, 64)}


def distribution_units(run, name, S=8192, seed=20260101):
  """The worst count deviation, in units of sqrt(S p (1 - p)) + 1, over all
  paths of one of DISTRIBUTIONS (weights N(0, 1)); run(context, W, nf, S,
  seed) -> labels [1, S, T]."""
  import collections
  rng = np.random.default_rng(7)
  make, T, npaths = DISTRIBUTIONS[name]
  context = make(rng)
  table = table_of(context)
  C, V = table.shape
  W = rng.standard_normal([1, T, C, V + 1]).astype(np.float32)
  probs = path_probabilities(W[0], table, T)
  assert len(probs) == npaths
  labels = run(context, W, [T], S, seed)
  counts = collections.Counter(tuple(int(y) for y in row) for row in labels[0])
  assert set(counts) <= set(probs)
  units = count_units([counts[s] for s in probs], list(probs.values()), S)
  print(f'{name}: worst path count deviation {units:.2f} units')
  return units


def check_paths(W, nf, table, labels, weights, log_z):
  """Every sampled path walks the table from state 0, is 0 on padding frames
  and on unsampled utterances, and its weight is the float64 sum of W along
  it within T 2^-23 sum |w_arc|."""
  B, S, T = labels.shape
  V = table.shape[1]
  assert labels.min() >= 0 and labels.max() <= V
  for b in range(B):
    n = min(max(int(nf[b]), 0), T)
    for s in range(S):
      assert not labels[b, s, n:].any()
      if not np.isfinite(log_z[b]):
        assert not labels[b, s].any() and weights[b, s] == -np.inf
        continue
      w, mag = path_weight(np.asarray(W[b], np.float64), labels[b, s, :n], table)
      assert np.isfinite(weights[b, s])
      assert abs(float(weights[b, s]) - w) <= n * 2.0**-23 * mag, (b, s, weights[b, s], w)
