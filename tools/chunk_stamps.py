"""Diagnostic: s_memtime marks per phase-C workgroup (diagnostic build:
make diag; LT_LIB_PATH=build/diag/liblt_lattice_diag.so). Prints the median
and 90th percentile of each segment in cycles, and the spread of start
times. The head ("DMA+tables", marks 0 -> 1) is also split at mark 6 (wave 0
has its progress words, frame offsets and verdict; 6 -> 1 is the rest of the
W DMA and the staging barrier) and, for libraries that still build the gather
tables per chunk, at mark 7 (past the barrier that hands the labels to every
wave). A second call with LT_CK_DBG=256 marks phase A's
chunk waves instead: 0 -> 1 labels and offsets, 1 -> 4 the first frame's
arrival, 4 -> 2 the frames, 2 -> 3 the record's stores."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault('LT_LIB_PATH', os.path.join(ROOT, 'build/diag/liblt_lattice_diag.so'))
from last_torch_amd import _native  # noqa: E402

B, T, U, V = int(os.environ.get('B', 64)), 1000, 100, 32
g = torch.Generator(device='cuda')
g.manual_seed(0)
W = torch.randn([B, T, V + 1, V + 1], generator=g, device='cuda')
nf = torch.full([B], T, dtype=torch.int32, device='cuda')
lab = torch.randint(1, V + 1, [B, U], generator=g, device='cuda', dtype=torch.int32)
nl = torch.full([B], U, dtype=torch.int32, device='cuda')
st = torch.zeros([B * 200 * 16], dtype=torch.int64, device='cuda')
for _ in range(3):
  _native.loss_grad(W, nf, lab, nl, V, 1, False)
torch.cuda.synchronize()
os.environ['LT_CK_STAMPS'] = hex(st.data_ptr())
_native.loss_grad(W, nf, lab, nl, V, 1, False)
torch.cuda.synchronize()
del os.environ['LT_CK_STAMPS']
if os.environ.get('LT_CK_LDS_PAD'):
  e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
  e0.record()
  for _ in range(10):
    _native.loss_grad(W, nf, lab, nl, V, 1, False)
  e1.record()
  torch.cuda.synchronize()
  print(f'LDS pad {os.environ["LT_CK_LDS_PAD"]}: {e0.elapsed_time(e1) / 10:.3f} ms per call')
s = st.cpu().numpy().reshape(-1, 8)
# the chunk workgroups: a row per block of the launch, the walking workgroups
# in front of them (when the launch finishes the walks) leave mark 1 empty
blk = np.nonzero((s[:, 0] > 0) & (s[:, 1] > 0))[0]
s = s[blk]
segs = [('DMA+tables', 0, 1), (' to poll end', 0, 6), (' poll->staging', 6, 1), (' to labels', 6, 7),
        (' labels->stag.', 7, 1),
        ('nw + E', 1, 5), ('recursions', 5, 2), ('marginals', 2, 3),
        ('dW stream', 3, 4)]


def report(s, head):
  for nm, i, j in segs:
    if not s[:, j].any() or not s[:, i].any():
      continue
    d = s[:, j] - s[:, i]
    print(f'{head}{nm:15s} median {np.median(d):8.0f}  p90 {np.percentile(d, 90):8.0f} cycles')
  tot = s[:, 4] - s[:, 0]
  print(f'{head}{"total":15s} median {np.median(tot):8.0f}  p90 {np.percentile(tot, 90):8.0f}; '
        f'workgroups {len(s)}')


report(s, '')
print(f'span {s[:, 4].max() - s[:, 0].min()} cycles')
# the marks are wave 0's, whose recursion rotates with the block (role
# (wave + (block >> 3)) & 3, so (block >> 3) & 3 for wave 0): per role, `recursions` is that chain's own
# length and `marginals` what follows it up to the workgroup's last barrier
for role, nm in enumerate(('den alpha', 'den beta', 'num alpha', 'num beta')):
  sel = ((blk >> 3) & 3) == role
  if sel.any():
    report(s[sel], f'[{nm:9s}] ')

# phase A's chunk waves (LT_CK_DBG bit 256: their marks instead of phase C's),
# eight words per chunk behind phase C's B * K rows
K = -(-T // 6)  # the plan's L at this shape
st.zero_()
os.environ['LT_CK_STAMPS'] = hex(st.data_ptr())
os.environ['LT_CK_DBG'] = '256'
_native.loss_grad(W, nf, lab, nl, V, 1, False)
torch.cuda.synchronize()
del os.environ['LT_CK_STAMPS'], os.environ['LT_CK_DBG']
sa = st.cpu().numpy()[B * K * 8:B * K * 16].reshape(-1, 8)
sa = sa[(sa[:, 0] > 0) & (sa[:, 3] > 0)]
for nm, i, j in (('labels+offsets', 0, 1), ('first frame', 1, 4), ('frames', 4, 2), ('record', 2, 3),
                 ('total', 0, 3)):
  d = sa[:, j] - sa[:, i]
  print(f'[phase A] {nm:14s} median {np.median(d):8.0f}  p90 {np.percentile(d, 90):8.0f} cycles'
        + (f'; chunk waves {len(sa)}' if nm == 'total' else ''))
