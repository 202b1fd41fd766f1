"""Shared helper of the forced-alignment tests: turns a dense one-hot string
gradient (the reference's autograd through _string_forward in MaxTropical, or
the pinned oracle's tab_dist_grad) into RecognitionLattice.align's outputs,
and loads the fixtures that carry such gradients."""
import os

import numpy as np

from golden_cases import GOLDEN

CASES = sorted(f[len('grads_'):-4] for f in os.listdir(GOLDEN) if f.startswith('grads_'))


def load(name):
  with np.load(os.path.join(GOLDEN, name + '.npz')) as z:
    d = {k: z[k] for k in z.files}
  with np.load(os.path.join(GOLDEN, 'grads_' + name + '.npz')) as z:
    d.update({k: z[k] for k in z.files})
  d['K'] = int(d['K']) if 'K' in d else 0
  return d


def compact(dW, dist, labels, num_labels, num_frames, K):
  """(alignment_labels [B, T*A], label_frames [B, U]) of the path marked in
  dW [B, T, C, V+1]: a frame's lexical count is round(dW[b, t, :, 1:].sum());
  u walks upward from 0, filling the frame's slots with the true labels and
  label_frames with the frame. Rows of -inf distance are all 0 / -1.

  Asserts what makes the reading unambiguous, so a broken reference cannot
  pass silently: on a finite row one arc per live frame (FrameDependent) or
  one blank plus at most K lexical arcs (FrameLabelDependent), nothing on
  padding frames, and the lexical total equals num_labels."""
  dW = np.asarray(dW, np.float64)
  B, T, _, R = dW.shape
  U = labels.shape[1]
  A = K + 1 if K else 1
  out = np.zeros((B, T * A), np.int64)
  frames = np.full((B, U), -1, np.int64)
  for b in range(B):
    if not dist[b] > -np.inf:
      continue
    nf = int(np.clip(num_frames[b], 0, T))
    u = 0
    for t in range(T):
      blank = int(round(dW[b, t, :, 0].sum()))
      lex = int(round(dW[b, t, :, 1:].sum()))
      assert dW[b, t].sum() == blank + lex
      if t >= nf:
        assert blank == 0 and lex == 0, (b, t)
      elif K == 0:
        assert blank + lex == 1, (b, t, blank, lex)
      else:
        assert blank == 1 and 0 <= lex <= K, (b, t, blank, lex)
      for i in range(lex):
        y = int(labels[b, u])
        out[b, t * A + i] = y if 1 <= y <= R - 1 else 0
        frames[b, u] = t
        u += 1
    assert u == int(num_labels[b]), (b, u, int(num_labels[b]))
  return out, frames
