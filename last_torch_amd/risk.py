"""Path costs for minimum-risk training (not in the reference).

``edit_distance`` is the unit-cost Levenshtein distance of hypothesis label
sequences -- alignment labels as ``RecognitionLattice.sample`` returns them --
against reference transcripts: the default cost of
``RecognitionLattice.sampled_risk``. ROCm tensors run lt_edit_distance
(include/lt_paths.h, one wave per hypothesis); CPU tensors, and references
past the kernel's 1023 labels, run the torch restatement
``cpu.edit_distance`` on the tensors' device.
"""
import torch

from last_torch_amd import _native
from last_torch_amd import cpu


def edit_distance(hyp_labels: torch.Tensor, hyp_num_frames, ref_labels: torch.Tensor,
                  ref_num_labels: torch.Tensor) -> torch.Tensor:
  """Levenshtein distance int32 [batch..., S] of hyp_labels [batch..., S, T]
  against ref_labels [batch..., U].

  Tokens are the values > 0: blanks (0) in an alignment and zero epsilons in a
  transcript are skipped, as are hypothesis positions t >= hyp_num_frames
  [batch...] (None: every position counts) and reference positions
  u >= ref_num_labels [batch...]. Substitution, insertion and deletion each
  cost 1. ref_num_labels outside [0, U] gives -1 for that utterance.
  """
  hyp_labels = torch.as_tensor(hyp_labels)
  ref_labels = torch.as_tensor(ref_labels)
  if hyp_labels.ndim < 2:
    raise ValueError(f'hyp_labels should be [batch..., S, T], got {tuple(hyp_labels.shape)}')
  batch_dims = tuple(hyp_labels.shape[:-2])
  if tuple(ref_labels.shape[:-1]) != batch_dims:
    raise ValueError('ref_labels and hyp_labels have different batch_dims: '
                     f'{tuple(ref_labels.shape[:-1])} vs {batch_dims}')
  if tuple(torch.as_tensor(ref_num_labels).shape) != batch_dims:
    raise ValueError('ref_num_labels and hyp_labels have different batch_dims: '
                     f'{tuple(torch.as_tensor(ref_num_labels).shape)} vs {batch_dims}')
  S, T = hyp_labels.shape[-2:]
  U = ref_labels.shape[-1]
  B = 1
  for d in batch_dims:
    B *= d
  dev = hyp_labels.device
  if not dev.type == 'cuda' and ref_labels.is_cuda:
    dev = ref_labels.device
  hyp = hyp_labels.to(dev).reshape(B, S, T)
  ref = ref_labels.to(dev).reshape(B, U)
  nl = torch.as_tensor(ref_num_labels).to(dev).reshape(B)
  nf = None if hyp_num_frames is None else torch.as_tensor(hyp_num_frames).to(dev).reshape(B)
  if S == 0 or B == 0:
    dist = torch.zeros([B, S], dtype=torch.int32, device=dev)
  elif dev.type == 'cuda' and _native.edit_distance_supported(U):
    dist = _native.edit_distance(hyp, nf, ref, nl, want_length=False)[0]
  else:
    dist = cpu.edit_distance(hyp, nf, ref, nl)[0]
  return dist.reshape(*batch_dims, S).to(hyp_labels.device)
