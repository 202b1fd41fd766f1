"""Recognition lattice (mirrors last_torch/lattices.py).

``RecognitionLattice`` keeps the reference's constructor and methods
(lattices.py:103-247, 250-799). Each method materialises the frame's arc
weights once through the ``WeightFn`` plugin as a contiguous
[B, T, C, V+1] tensor and hands it to the HIP kernels in
``liblt_lattice.so`` through ``_native`` (C ABI: include/lt_lattice.h):

  forward         -> lt_loss_grad (loss + dW, the design per shape);
                     lt_scale_grad in the backward; lt_loss_forward without grad
  _forward        -> lt_den_forward (Log, MaxTropical, Real);
                     autograd: lt_den_backward (Log) / lt_viterbi arcs (Max) /
                     lt_table_den_backward (Real)
  _forward_backward -> lt_den_forward + lt_den_backward
  _backward       -> lt_den_backward marginals, streamed to the callback
  _string_forward -> lt_num_forward; autograd: lt_loss_backward (Log) /
                     lt_table_num_backward (MaxTropical, Real)
  shortest_path   -> lt_viterbi
  align           -> lt_table_align (forced alignment; not in the reference);
                     past its range lt_table_num_backward (Max) compacted
  align_posteriors -> lt_table_align_posteriors (emission posteriors of the
                     label string; not in the reference); past its range the
                     torch restatement (cpu.align_posteriors) on the device
  align_expectation -> lt_table_align_expectation (expected value of a path
                     quantity over the transcript's alignments, with the
                     posteriors and covariances its backward needs; not in the
                     reference) + lt_table_string_scatter in the backward; past
                     its range cpu.align_expectation on the device
  sample          -> lt_den_forward / lt_table_forward (Log) + lt_table_sample
                     (paths from the posterior; not in the reference)
  beam_search     -> lt_table_beam_search (the N best label sequences by
                     prefix beam search; not in the reference); past its range
                     cpu.beam_search on the device
  path_weights    -> lt_table_path_score (the weight of given alignment paths;
                     not in the reference) + lt_table_path_scatter in the
                     backward; past its range cpu.path_weights on the device
  sampled_risk    -> sample's calls + lt_table_path_score + lt_edit_distance
                     (minimum-risk training from sampled paths; not in the
                     reference); backward: lt_table_path_scatter, and
                     lt_den_backward / lt_table_den_backward only at S = 1
  expectation     -> lt_table_expectation (posterior mean of arc values with
                     its gradients; not in the reference), also behind
                     entropy(differentiable=True)

The device of the arc weights picks the implementation, as in the
reference: ROCm tensors run the HIP kernels (FrameDependent and
FrameLabelDependent alignments, FullNGram or any next-state table), CPU
tensors the C++ host twin (``liblt_lattice_cpu.so``, include/lt_lattice_cpu.h:
``forward`` and ``shortest_path`` of FullNGram x FrameDependent) or the
PyTorch restatement in ``cpu.py`` (every other method and lattice). There is no
fallback between the two: a ROCm tensor never runs on the CPU, and a missing
HIP library raises. Arbitrary batch dims are flattened (the reference's
``_string_forward`` supports only one, D13).
"""
from collections.abc import Callable, Sequence
from typing import Any, Generic, Optional, Protocol, TypeVar

import torch
import torch.nn as nn

from last_torch_amd import _native
from last_torch_amd import _native_cpu
from last_torch_amd import alignments
from last_torch_amd import cpu
from last_torch_amd import contexts
from last_torch_amd import risk as risk_lib
from last_torch_amd import semirings
from last_torch_amd import weight_fns

T = TypeVar('T')

_SEMIRING_IDS = {'Log': _native.SEMIRING_LOG, 'MaxTropical': _native.SEMIRING_MAX,
                 'Real': _native.SEMIRING_REAL}


def _semiring_id(semiring) -> int:
  name = getattr(semiring, 'name', None)
  if name not in _SEMIRING_IDS:
    raise NotImplementedError(f'lattice kernels support Log, MaxTropical and Real, got {semiring!r}')
  return _SEMIRING_IDS[name]


def _compute_device(W, *tensors) -> torch.device:
  """The arc weights' device (a ROCm device if any input is on one): ROCm
  -> HIP kernels, CPU -> cpu.py."""
  for t in (W, *tensors):
    if isinstance(t, torch.Tensor) and t.is_cuda:
      return t.device
  return torch.device('cpu')


def _lengths(x, batch_numel, device) -> torch.Tensor:
  return torch.as_tensor(x).reshape(batch_numel).to(device=device, dtype=torch.int32)


def _kernel_weights(W: torch.Tensor) -> torch.Tensor:
  if W.dtype not in (torch.float32, torch.bfloat16):
    W = W.float()
  W = W.contiguous()
  if W.data_ptr() % 16:
    W = W.clone()
  return W


class _LossFn(torch.autograd.Function):
  """loss = log_z - num (or -num), lattices.py:131-183, on the HIP kernels.

  With a gradient wanted, the forward is ONE lt_loss_grad call -- the loss
  and d(sum loss)/dW together, in whichever design lt_loss_grad_design picks
  for the shape (the chunked scan at the bench's B=64, the checkpointing
  pipe + marginal pass at B=256, the trigram's checkpointing pair): exactly
  what bench.py times, with the chunked path's per-frame certificate deciding
  which utterances the frame-serial kernels redo. The backward scales that
  dW by the incoming per-utterance gradient in place (lt_scale_grad: no work
  where it is 1); a second backward (retain_graph) recomputes it. Without a
  gradient only the loss is computed (lt_loss_forward)."""

  @staticmethod
  def forward(ctx, W, nf, labels, nl, V, n, local):
    ctx.cfg = (V, n, local)
    if not ctx.needs_input_grad[0]:
      return _native.loss_forward(W, nf, labels, nl, V, n, local, want_alpha=False)[0]
    loss, _, _, dW = _native.loss_grad(W, nf, labels, nl, V, n, local)
    ctx.dW = dW
    ctx.save_for_backward(W, nf, labels, nl)
    return loss

  @staticmethod
  def backward(ctx, g):
    V, n, local = ctx.cfg
    dW = ctx.dW
    ctx.dW = None
    if dW is None:  # a second backward through the same graph
      W, nf, labels, nl = ctx.saved_tensors
      dW = _native.loss_grad(W, nf, labels, nl, V, n, local)[3]
    _native.scale_grad(dW, g.float().contiguous(), V, n)
    return dW, None, None, None, None, None, None


class _CpuLossFn(torch.autograd.Function):
  """The same loss on host tensors through the C++ twin (lt_cpu_loss_grad,
  include/lt_lattice_cpu.h): FullNGram x FrameDependent, loss and
  d(sum loss)/dW in one call on the host thread pool; the backward scales
  it by the incoming gradient."""

  @staticmethod
  def forward(ctx, W, nf, labels, nl, V, n, local):
    want = ctx.needs_input_grad[0]
    loss, _, _, dW = _native_cpu.loss_grad(W, nf, labels, nl, V, n, local, with_grad=want)
    ctx.dW = dW
    if want:
      ctx.save_for_backward(W, nf, labels, nl)
    ctx.cfg = (V, n, local)
    return loss

  @staticmethod
  def backward(ctx, g):
    if torch.is_grad_enabled():
      # create_graph (higher-order gradients): the twin's dW is a constant,
      # so the differentiable backward goes through cpu.py's autograd
      W, nf, labels, nl = ctx.saved_tensors
      V, n, local = ctx.cfg
      loss = cpu.loss(W, nf.long(), labels, nl.long(),
                      contexts.FullNGram(vocab_size=V, context_size=n),
                      alignments.FrameDependent(), local)
      fin = torch.isfinite(loss)
      (dW,) = torch.autograd.grad(loss, W, torch.where(fin, g, torch.zeros_like(g)),
                                  create_graph=True)
      return dW, None, None, None, None, None, None
    dW = ctx.dW
    ctx.dW = None
    if dW is None:  # a second backward through the same graph
      W, nf, labels, nl = ctx.saved_tensors
      dW = _native_cpu.loss_grad(W, nf, labels, nl, *ctx.cfg)[3]
    return (dW * g.to(dW.dtype)[:, None, None, None], None, None, None, None, None, None)


class _TableLossFn(torch.autograd.Function):
  """loss for the general lattices (lt_table_loss_grad): any next-state
  table, FrameDependent or FrameLabelDependent(K). The gradient of
  sum(loss) comes with the forward; the backward scales it."""

  @staticmethod
  def forward(ctx, W, nf, labels, nl, graph, local):
    want = ctx.needs_input_grad[0]
    loss, _, _, dW = _native.table_loss_grad(graph, W, nf, labels, nl, local, want_grad=want)
    ctx.dW = dW
    return loss

  @staticmethod
  def backward(ctx, g):
    dW = ctx.dW
    if dW is None:
      raise RuntimeError('the lattice loss gradient was already consumed: backward through '
                         'RecognitionLattice.forward twice is not supported (call it again)')
    ctx.dW = None
    return (dW * g.to(dW.dtype)[:, None, None, None], None, None, None, None, None)


class _DenFn(torch.autograd.Function):
  """Denominator shortest distance; gradient = arc marginals (Log) or the
  best-path indicator (MaxTropical)."""

  @staticmethod
  def forward(ctx, W, nf, V, n, sid, graph=None):
    dist, alpha = _native.den_forward(W, nf, V, n, sid, want_alpha=True)
    ctx.save_for_backward(W, nf, dist, alpha)
    ctx.cfg = (V, n, sid)
    ctx.graph = graph
    ctx.mark_non_differentiable(alpha)
    return dist, alpha

  @staticmethod
  def backward(ctx, g, g_alpha):
    del g_alpha  # alpha_0..T-1 is a checkpoint, not differentiated
    W, nf, dist, alpha = ctx.saved_tensors
    V, n, sid = ctx.cfg
    g = g.float().contiguous()
    if sid == _native.SEMIRING_LOG:
      dW = _native.den_backward(W, nf, dist, alpha, g, V, n)
    elif sid == _native.SEMIRING_MAX:
      _, _, dW = _native.viterbi(W, nf, V, n, _native.LABELS_TRUE, grad=g, want_arcs=True)
    else:
      # Real (semirings.py:143-173, plain-arithmetic autograd in the
      # reference): d dist / dW = alpha * beta' from the general table
      # kernels on FullNGram.next_state_table() (the same state numbering)
      if ctx.graph is None:
        raise NotImplementedError('Real-semiring gradients need the lattice graph')
      dW = _native.table_den_backward(ctx.graph, W, nf, sid, dist, alpha, g)
    return dW, None, None, None, None, None


class _TableDenFn(torch.autograd.Function):
  """_forward's distance on the general table kernels (any next-state table,
  FrameDependent or FrameLabelDependent); gradient lt_table_den_backward: the
  arc marginals (Log), alpha * beta' (Real), the best path's arcs
  (MaxTropical)."""

  @staticmethod
  def forward(ctx, W, nf, graph, sid):
    dist, alpha = _native.table_forward(graph, W, nf, sid, want_alpha=True)
    ctx.save_for_backward(W, nf, dist, alpha)
    ctx.graph, ctx.sid = graph, sid
    ctx.mark_non_differentiable(alpha)
    return dist, alpha

  @staticmethod
  def backward(ctx, g, g_alpha):
    del g_alpha
    W, nf, dist, alpha = ctx.saved_tensors
    dW = _native.table_den_backward(ctx.graph, W, nf, ctx.sid, dist, alpha, g.float())
    return dW, None, None, None


class _ExpectFn(torch.autograd.Function):
  """(E, log_z) of include/lt_expect.h on the table kernels: the forward is
  ONE lt_table_expectation call that also writes the gradient tensors the
  inputs need (marg = dE/dvalues = d log_z/dW, cov = dE/dW); the backward
  combines them with the incoming gradients. A second backward (retain_graph)
  recomputes them. Not twice differentiable."""

  @staticmethod
  def forward(ctx, W, values, nf, graph):
    need_w, need_v = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    expected, log_z, marg, cov = _native.table_expectation(
        graph, W, values, nf, want_marg=need_w or need_v, want_cov=need_w)
    ctx.graph, ctx.marg, ctx.cov = graph, marg, cov
    ctx.save_for_backward(W, values, nf)
    return expected, log_z

  @staticmethod
  def backward(ctx, g_e, g_z):
    W, values, nf = ctx.saved_tensors
    need_w, need_v = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    marg, cov = ctx.marg, ctx.cov
    ctx.marg = ctx.cov = None
    if marg is None and (need_w or need_v):  # a second backward through the same graph
      _, _, marg, cov = _native.table_expectation(ctx.graph, W, values, nf,
                                                  want_marg=True, want_cov=need_w)
    g_e = g_e.float()[:, None, None, None]
    dW = dv = None
    if need_w:
      dW = (g_e * cov + g_z.float()[:, None, None, None] * marg).to(W.dtype)
    if need_v:
      dv = (g_e * marg).to(values.dtype)
    return dW, dv, None, None


class _AlignExpectFn(torch.autograd.Function):
  """(expected, log_prob) of include/lt_string_expect.h: the forward is ONE
  lt_table_align_expectation call that also writes what the inputs' gradients
  need (the posteriors emission / blank_occ = d expected / d values = d
  log_prob / d string weights, the covariances = d expected / d string
  weights); the backward combines them with the incoming gradients in string
  coordinates and ONE lt_table_string_scatter call makes the dense dW. A
  second backward (retain_graph) recomputes them. Not twice differentiable."""

  @staticmethod
  def forward(ctx, W, lv, bv, nf, lab, nl, graph):
    need_w, need_l, need_b = ctx.needs_input_grad[:3]
    expected, log_prob, *grads = _native.table_align_expectation(
        graph, W, lv, bv, nf, lab, nl, want_post=need_w or need_l or need_b, want_cov=need_w)
    ctx.graph, ctx.grads = graph, grads
    ctx.save_for_backward(W, lv, bv, nf, lab, nl)
    return expected, log_prob

  @staticmethod
  def backward(ctx, g_e, g_lp):
    W, lv, bv, nf, lab, nl = ctx.saved_tensors
    need_w, need_l, need_b = ctx.needs_input_grad[:3]
    grads, ctx.grads = ctx.grads, None
    if grads is None and (need_w or need_l or need_b):  # a second backward through the same graph
      grads = _native.table_align_expectation(ctx.graph, W, lv, bv, nf, lab, nl, want_post=True,
                                              want_cov=need_w)[2:]
    emission, blank_occ, cov_lex, cov_blank = grads if grads is not None else [None] * 4
    g_e = g_e.float()[:, None, None]
    dW = dl = db = None
    if need_w:
      g_lp = g_lp.float()[:, None, None]
      dW = _native.table_string_scatter(ctx.graph, W, g_e * cov_lex + g_lp * emission,
                                        g_e * cov_blank + g_lp * blank_occ, nf, lab,
                                        nl).to(W.dtype)
    if need_l:
      dl = (g_e * emission).to(lv.dtype)
    if need_b:
      db = (g_e * blank_occ).to(bv.dtype)
    return dW, dl, db, None, None, None, None


class _PathScoreFn(torch.autograd.Function):
  """The weights of given paths (include/lt_paths.h): the forward is ONE
  lt_table_path_score call that keeps the states it walked; the backward is
  ONE lt_table_path_scatter call that puts each path's incoming gradient on
  its arcs. A second backward (retain_graph) reuses the saved states."""

  @staticmethod
  def forward(ctx, W, nf, labels, graph):
    need = ctx.needs_input_grad[0]
    weight, states = _native.table_path_score(graph, W, nf, labels, want_states=need)
    ctx.graph = graph
    if need:
      ctx.save_for_backward(W, nf, labels, states)
    return weight

  @staticmethod
  def backward(ctx, g):
    W, nf, labels, states = ctx.saved_tensors
    dW = _native.table_path_scatter(ctx.graph, W, nf, labels, states, g.float())
    return dW.to(W.dtype), None, None, None


class _TableNumFn(torch.autograd.Function):
  """_string_forward on the general table kernels; Log gradient = the string
  marginals (lt_table_loss_grad with local normalisation gives -d num / dW)."""

  @staticmethod
  def forward(ctx, W, nf, labels, nl, graph, sid):
    num = _native.table_num_forward(graph, W, nf, labels, nl, sid)
    ctx.save_for_backward(W, nf, labels, nl)
    ctx.graph, ctx.sid = graph, sid
    return num

  @staticmethod
  def backward(ctx, g):
    W, nf, labels, nl = ctx.saved_tensors
    if ctx.sid != _native.SEMIRING_LOG:
      # MaxTropical: the best string-aligned path's arcs; Real: alpha * beta'
      # (lt_table_num_backward, the reference's autograd through
      # semirings.py:143-173 / 354-401)
      _, dW = _native.table_num_backward(ctx.graph, W, nf, labels, nl, ctx.sid, g.float())
      return dW, None, None, None, None, None
    _, _, _, dW = _native.table_loss_grad(ctx.graph, W, nf, labels, nl, True)
    # an unreachable string has num = -inf and dW = 0 already
    return dW * (-g).to(dW.dtype)[:, None, None, None], None, None, None, None, None


class _NumFn(torch.autograd.Function):
  """Numerator (string) shortest distance; gradient = the string marginals
  (Log), the best string-aligned path's arcs (MaxTropical) or alpha * beta'
  (Real)."""

  @staticmethod
  def forward(ctx, W, nf, labels, nl, V, n, sid, graph=None):
    num, an = _native.num_forward(W, nf, labels, nl, V, n, sid,
                                  want_alpha=sid == _native.SEMIRING_LOG)
    ctx.save_for_backward(W, nf, labels, nl, num, an)
    ctx.cfg = (V, n, sid)
    ctx.graph = graph
    return num

  @staticmethod
  def backward(ctx, g):
    W, nf, labels, nl, num, an = ctx.saved_tensors
    V, n, sid = ctx.cfg
    if sid != _native.SEMIRING_LOG:
      # the general string-gradient kernel on FullNGram.next_state_table()
      # (the same state numbering): lt_table_num_backward
      if ctx.graph is None:
        raise NotImplementedError('MaxTropical / Real string gradients need the lattice graph')
      _, dW = _native.table_num_backward(ctx.graph, W, nf, labels, nl, sid, g.float())
      return dW, None, None, None, None, None, None, None
    # local-norm loss backward gives -grad * num marginals; feed -g.
    dW = _native.loss_backward(W, nf, labels, nl, None, num, None, an,
                               (-g).float().contiguous(), V, n, True)
    return dW, None, None, None, None, None, None, None


class RecognitionLattice(nn.Module, Generic[T]):
  """GNAT recognition lattice = context dependency x alignment lattice, with
  arc weights from a weight function (lattices.py:35-116)."""

  def __init__(self, context: contexts.ContextDependency,
               alignment: alignments.TimeSyncAlignmentLattice,
               weight_fn_cacher_factory: Callable[[contexts.ContextDependency],
                                                  weight_fns.WeightFnCacher[T]],
               weight_fn_factory: Callable[[contexts.ContextDependency], weight_fns.WeightFn[T]]):
    super().__init__()
    self.context = context
    self.alignment = alignment
    self.weight_fn_cacher_factory = weight_fn_cacher_factory
    self.weight_fn_factory = weight_fn_factory
    self.weight_fn_cacher = weight_fn_cacher_factory(context)
    self.weight_fn = weight_fn_factory(context)

  # -- helpers -------------------------------------------------------------
  def _table_path(self) -> bool:
    """False: FullNGram x FrameDependent, the tuned kernels (lt_lattice.hip,
    lt_pipe.hip). True: any other context (through its next-state table)
    with FrameDependent or FrameLabelDependent -- the general table kernels
    (lt_table.hip)."""
    if not isinstance(self.alignment, (alignments.FrameDependent,
                                       alignments.FrameLabelDependent)):
      raise NotImplementedError(f'lattice kernels implement FrameDependent and '
                                f'FrameLabelDependent alignments, got '
                                f'{type(self.alignment).__name__}')
    return not (isinstance(self.context, contexts.FullNGram) and
                isinstance(self.alignment, alignments.FrameDependent))

  def _graph(self, device) -> '_native.TableGraph':
    cache = self.__dict__.setdefault('_graphs', {})
    key = str(device)
    if key not in cache:
      if isinstance(self.context, contexts.NextStateTable):
        table = self.context.next_state_table
      elif hasattr(self.context, 'next_state_table'):
        table = self.context.next_state_table()
      else:
        raise NotImplementedError(f'{type(self.context).__name__} has no next-state table')
      K = (self.alignment.max_expansions
           if isinstance(self.alignment, alignments.FrameLabelDependent) else 0)
      cache[key] = _native.TableGraph(table, K, device)
    return cache[key]

  def _ngram(self) -> tuple[int, int]:
    if not isinstance(self.context, contexts.FullNGram):
      raise NotImplementedError(f'lattice kernels implement FullNGram contexts, got '
                                f'{type(self.context).__name__}')
    if not isinstance(self.alignment, alignments.FrameDependent):
      raise NotImplementedError(f'lattice kernels implement FrameDependent alignments, got '
                                f'{type(self.alignment).__name__}')
    return self.context.vocab_size, self.context.context_size

  def build_cache(self) -> T:
    """Builds the weight function cache (lattices.py:118-129)."""
    return self.weight_fn_cacher()

  def arc_weights(self, cache: T, frames: torch.Tensor) -> torch.Tensor:
    """All arc weights [batch..., T, C, V+1]: [..., 0] blank, [..., y] label y.

    Calls ``weight_fn(cache, frame)`` vectorised over time (the reference
    vmaps weight_fn the same way, lattices.py:308-313), falling back to one
    call per frame for weight functions vmap cannot trace.
    """
    tdim = frames.ndim - 2
    if getattr(self.weight_fn, 'time_batched', False):
      # the weight function takes any leading dims (JointWeightFn's
      # matrix-core producer: one launch for every frame)
      if hasattr(self.weight_fn, 'forward_joint'):
        return self.weight_fn.forward_joint(cache, frames)
      blank, lexical = self.weight_fn(cache, frames)
      return torch.cat([blank[..., None], lexical], dim=-1)

    def frame_weights(frame):
      blank, lexical = self.weight_fn(cache, frame)
      return torch.cat([blank[..., None], lexical], dim=-1)

    try:
      return torch.vmap(frame_weights, in_dims=tdim, out_dims=tdim, randomness='same')(frames)
    except Exception:  # pylint: disable=broad-except
      return torch.stack([frame_weights(frames[..., t, :]) for t in range(frames.shape[-2])],
                         dim=tdim)

  def _prepare(self, cache, frames, num_frames):
    batch_dims = tuple(num_frames.shape)
    if tuple(frames.shape[:-2]) != batch_dims:
      raise ValueError('frames and num_frames have different batch_dims: '
                       f'{tuple(frames.shape[:-2])} vs {batch_dims}')
    V, n = self._ngram() if not self._table_path() else (None, None)
    if cache is None:
      cache = self.weight_fn_cacher()
    W = self.arc_weights(cache, frames)
    B = 1
    for d in batch_dims:
      B *= d
    dev = _compute_device(W, frames, num_frames)
    W = W.to(dev).reshape(B, *W.shape[-3:])
    W = _kernel_weights(W) if dev.type == 'cuda' else W.float()
    nf = _lengths(num_frames, B, dev)
    if dev.type != 'cuda':
      nf = nf.long()
    return W, nf, batch_dims, B, V, n, cache

  @staticmethod
  def _home(x, like):
    return x.to(like.device) if isinstance(like, torch.Tensor) else x

  # -- public API ------------------------------------------------------------
  def forward(self, frames: torch.Tensor, num_frames: torch.Tensor, labels: torch.Tensor,
              num_labels: torch.Tensor, cache: Optional[T] = None) -> torch.Tensor:
    """Negative sequence log-probability -log P(labels | frames)
    (lattices.py:131-183); differentiable w.r.t. the weight function."""
    batch_dims = tuple(num_frames.shape)
    if tuple(frames.shape[:-2]) != batch_dims:
      raise ValueError('frames and num_frames have different batch_dims: '
                       f'{tuple(frames.shape[:-2])} vs {batch_dims}')
    if tuple(labels.shape[:-1]) != batch_dims:
      raise ValueError('labels and num_frames have different batch_dims: '
                       f'{tuple(labels.shape[:-1])} vs {batch_dims}')
    if tuple(num_labels.shape) != batch_dims:
      raise ValueError('num_labels and num_frames have different batch_dims: '
                       f'{tuple(num_labels.shape)} vs {batch_dims}')
    fused = self._fused_joint_loss(cache, frames, num_frames, labels, num_labels)
    if fused is not None:
      return self._home(fused.reshape(batch_dims), frames)
    W, nf, batch_dims, B, V, n, cache = self._prepare(cache, frames, num_frames)
    lab = torch.as_tensor(labels).reshape(B, -1).to(device=W.device, dtype=torch.int32)
    nl = _lengths(num_labels, B, W.device)
    local = isinstance(self.weight_fn, weight_fns.LocallyNormalizedWeightFn)
    if W.device.type == 'cpu':
      if not self._table_path() and _native_cpu.available():
        loss = _CpuLossFn.apply(W, nf, lab.contiguous(), nl, V, n, local)
      else:
        loss = cpu.loss(W, nf, lab, nl.long(), self.context, self.alignment, local)
    elif self._table_path():
      loss = _TableLossFn.apply(W, nf, lab.contiguous(), nl, self._graph(W.device), local)
    else:
      loss = _LossFn.apply(W, nf, lab.contiguous(), nl, V, n, local)
    return self._home(loss.reshape(batch_dims), frames)

  def _fused_joint_loss(self, cache, frames, num_frames, labels, num_labels):
    """The loss through the fused joint weight function + lattice kernels
    (JointWeightFn.fused_lattice_loss, lt_loss_joint_forward / _backward) when
    the weight function takes that path: FullNGram x FrameDependent on a ROCm
    device, one batch dim; else None."""
    fn = getattr(self.weight_fn, 'fused_lattice_loss', None)
    if fn is None or self._table_path() or frames.ndim != 3 or not frames.is_cuda:
      return None
    if cache is None:
      cache = self.weight_fn_cacher()
    dev = frames.device
    B = frames.shape[0]
    nf = _lengths(num_frames, B, dev)
    lab = torch.as_tensor(labels).reshape(B, -1).to(device=dev, dtype=torch.int32).contiguous()
    nl = _lengths(num_labels, B, dev)
    return fn(cache, frames, nf, lab, nl, self.context.vocab_size, self.context.context_size)

  def shortest_path(self, frames: torch.Tensor, num_frames: torch.Tensor,
                    cache: Optional[T] = None, label_convention: str = 'reference'):
    """Best alignment path (lattices.py:185-247).

    Returns (alignment_labels [batch..., T], num_alignment_labels, path_weights).
    ``label_convention='reference'`` (default) emits lexical label y as y-1
    exactly like the reference (lattices.py:242-244);
    ``'true'`` emits y. Unlike the reference, every utterance of a batch is
    decoded independently (D6).
    """
    conv = {'reference': _native.LABELS_REFERENCE, 'true': _native.LABELS_TRUE}[label_convention]
    W, nf, batch_dims, B, V, n, _ = self._prepare(cache, frames, num_frames)
    with torch.no_grad():
      if W.device.type == 'cpu' and not self._table_path() and _native_cpu.available():
        labels, weights, _ = _native_cpu.viterbi(W.detach(), nf, V, n, conv)
      elif W.device.type == 'cpu':
        labels, weights = cpu.viterbi(W, nf, self.context, self.alignment, label_convention)
      elif self._table_path():
        # A labels per frame: slot i = the (i+1)-th lexical label of the frame
        labels, weights = _native.table_viterbi(self._graph(W.device), W.detach(), nf, conv)
      else:
        labels, weights, _ = _native.viterbi(W.detach(), nf, V, n, conv)
    labels = self._home(labels.reshape(*batch_dims, -1), frames)
    num_alignment_labels = self.alignment.num_states() * num_frames
    return labels, num_alignment_labels, self._home(weights.reshape(batch_dims), frames)

  def align(self, frames: torch.Tensor, num_frames: torch.Tensor, labels: torch.Tensor,
            num_labels: torch.Tensor, cache: Optional[T] = None):
    """Forced alignment (not in the reference): the MaxTropical best path of
    the lattice intersected with the label string, i.e. on which frame each
    label is emitted. Ties: the blank term wins (FrameDependent), the fewest
    expansions win (FrameLabelDependent); labels outside 1..V are epsilons.

    Returns (alignment_labels [batch..., T*A], label_frames [batch..., U],
    path_weights [batch...]), A = alignment.num_states(): slot i of frame t
    holds the true label y of the (i+1)-th lexical arc the path takes in that
    frame (0 for an epsilon), else 0 -- shortest_path's slot layout, without a
    label convention (D5 is not reproduced); label_frames[u] is the frame on
    which the arc leaving string position u is taken, -1 for u >= num_labels;
    path_weights equals _string_forward(..., MaxTropical) bit for bit. An
    utterance of weight -inf (no path, -inf arcs, num_labels outside [0, U])
    is unaligned: all 0 / all -1.
    """
    batch_dims = tuple(num_frames.shape)
    if tuple(frames.shape[:-2]) != batch_dims:
      raise ValueError('frames and num_frames have different batch_dims: '
                       f'{tuple(frames.shape[:-2])} vs {batch_dims}')
    if tuple(labels.shape[:-1]) != batch_dims:
      raise ValueError('labels and num_frames have different batch_dims: '
                       f'{tuple(labels.shape[:-1])} vs {batch_dims}')
    if tuple(num_labels.shape) != batch_dims:
      raise ValueError('num_labels and num_frames have different batch_dims: '
                       f'{tuple(num_labels.shape)} vs {batch_dims}')
    W, nf, batch_dims, B, _, _, _ = self._prepare(cache, frames, num_frames)
    lab = torch.as_tensor(labels).reshape(B, -1).to(device=W.device, dtype=torch.int32).contiguous()
    nl = _lengths(num_labels, B, W.device)
    with torch.no_grad():
      W = W.detach()
      if W.device.type == 'cpu':
        out = cpu.align(W, nf, lab, nl.long(), self.context, self.alignment)
      else:
        graph = self._graph(W.device)
        # one launch (lt_table_align); past its range (U > 255, K > 15) the
        # dense string gradient, compacted
        if _native.table_align_supported(graph, W, lab):
          out = _native.table_align(graph, W, nf, lab, nl)
        else:
          out = self._align_dense(graph, W, nf, lab, nl)
    alignment_labels, label_frames, weights = out
    return (self._home(alignment_labels.reshape(*batch_dims, -1), frames),
            self._home(label_frames.reshape(*batch_dims, -1), frames),
            self._home(weights.reshape(batch_dims), frames))

  def align_posteriors(self, frames: torch.Tensor, num_frames: torch.Tensor,
                       labels: torch.Tensor, num_labels: torch.Tensor, cache: Optional[T] = None):
    """Soft forced alignment (not in the reference): with what probability is
    each label of the transcript emitted on each frame, given the transcript
    -- `align`'s question in the Log semiring. The definition is in
    include/lt_posterior.h: with alpha / beta the Log forward / backward
    vectors of the lattice intersected with the label string,

        emission[t, u] = exp(alpha_t[u] + lex_t[u] + beta_{t+1}[u+1] - log_prob)
                       = d log_prob / d lex_t[u],

    the posterior probability that the arc leaving string position u (the
    one that emits labels[u]) is taken on frame t; FrameLabelDependent sums
    the frame's expansion slots. Labels outside 1..V are epsilons.

    Returns (emission [batch..., T, U] float32, log_prob [batch...] float32),
    frame-major like the arc weights, so
    ``(arange(T)[:, None] * emission).sum(-2)`` is the expected emission frame
    of each label. log_prob equals _string_forward(..., Log) up to rounding.
    Two invariants hold for an aligned utterance (up to fp32 rounding):
    ``emission.sum(-2)[..., u] == 1`` for u < num_labels (every label is
    emitted exactly once), and on FrameDependent ``emission.sum(-1) <= 1``
    per frame (a frame emits at most one label). emission is exactly 0 for
    u >= num_labels and t >= num_frames. An utterance whose log_prob is not
    finite (no path, -inf arcs on every path, num_labels outside [0, U]) has
    log_prob = -inf and an all-zero emission, never NaN. No gradient flows
    through either output.

    ROCm tensors run one launch of lt_table_align_posteriors (FrameDependent,
    U <= 255, fp32 or bf16 weights); FrameLabelDependent or longer strings
    run the torch restatement (cpu.align_posteriors) on the tensors' own
    device; CPU tensors run it on the host.
    """
    batch_dims = tuple(num_frames.shape)
    if tuple(frames.shape[:-2]) != batch_dims:
      raise ValueError('frames and num_frames have different batch_dims: '
                       f'{tuple(frames.shape[:-2])} vs {batch_dims}')
    if tuple(labels.shape[:-1]) != batch_dims:
      raise ValueError('labels and num_frames have different batch_dims: '
                       f'{tuple(labels.shape[:-1])} vs {batch_dims}')
    if tuple(num_labels.shape) != batch_dims:
      raise ValueError('num_labels and num_frames have different batch_dims: '
                       f'{tuple(num_labels.shape)} vs {batch_dims}')
    W, nf, batch_dims, B, _, _, _ = self._prepare(cache, frames, num_frames)
    lab = torch.as_tensor(labels).reshape(B, -1).to(device=W.device, dtype=torch.int32).contiguous()
    nl = _lengths(num_labels, B, W.device)
    with torch.no_grad():
      W = W.detach()
      if W.device.type == 'cpu':
        out = cpu.align_posteriors(W, nf, lab, nl.long(), self.context, self.alignment)
      else:
        graph = self._graph(W.device)
        if _native.table_align_posteriors_supported(graph, W, lab):
          out = _native.table_align_posteriors(graph, W, nf, lab, nl)
        else:
          # the same restatement on the device: the walk reads the graph's
          # device copy of the next-state table, nothing visits the host
          out = cpu.align_posteriors(W, nf.long(), lab, nl.long(),
                                     contexts.NextStateTable(graph.table), self.alignment)
    emission, log_prob = out
    T_, U_ = W.shape[1], lab.shape[-1]
    return (self._home(emission.float().reshape(*batch_dims, T_, U_), frames),
            self._home(log_prob.float().reshape(batch_dims), frames))

  def align_expectation(self, frames: torch.Tensor, num_frames: torch.Tensor,
                        labels: torch.Tensor, num_labels: torch.Tensor,
                        lexical_values: torch.Tensor,
                        blank_values: Optional[torch.Tensor] = None, cache: Optional[T] = None):
    """Expected value of a path quantity over the alignments of a transcript
    (not in the reference): `expectation`'s question on the lattice
    intersected with the label string, differentiable, so it can be a loss
    term -- expected emission delay (lexical_values[t, u] = t), expected
    alignment cost against reference timestamps, the alignment entropy of one
    transcript (the string's own weights as values: log_prob - expected). The
    definition is in include/lt_string_expect.h. Values are given in string
    coordinates, the coordinates of `align_posteriors`:

        lexical_values [batch..., T, U]    the arc leaving string position u
                                           (the one that emits labels[u]) on frame t
        blank_values   [batch..., T, U+1]  the blank arc at position u on frame t
                                           (None: zeros)

        expected = sum_pi p(pi) sum_{a in pi} v_a,  p(pi) = exp(w(pi) - log_prob)
                 = sum_{t,u} emission[t,u] lexical_values[t,u]
                 + sum_{t,u} blank_occ[t,u] blank_values[t,u]

    over the alignment paths pi of the transcript, emission as
    `align_posteriors` returns it and blank_occ the same posterior of the
    blank arcs. Values may have any sign. Labels outside 1..V are epsilons.

    Returns (expected [batch...], log_prob [batch...]). Both are
    differentiable w.r.t. the weight function through the arc weights
    (d expected / d w_a is the covariance of the arc indicator with the path
    value), and `expected` also w.r.t. both value tensors: d expected / d
    lexical_values = emission, d expected / d blank_values = blank_occ. On
    ROCm tensors the gradients come from the forward's one
    lt_table_align_expectation call plus one lt_table_string_scatter call in
    the backward (FrameDependent, U <= 255, fp32 or bf16 weights) and are not
    twice differentiable; FrameLabelDependent or longer strings run
    cpu.align_expectation (plain autograd) on the tensors' own device; CPU
    tensors run it on the host. An arc of weight -inf contributes nothing and
    its value is ignored (NaN or inf there is harmless), as are values on
    frames t >= num_frames and positions past num_labels; an utterance whose
    log_prob is not finite (no path, -inf arcs on every path, num_labels
    outside [0, U]) gives log_prob = -inf, expected = 0 and zero gradients,
    never NaN; num_frames = 0 with num_labels = 0 gives (0, 0)."""
    batch_dims = tuple(num_frames.shape)
    if tuple(frames.shape[:-2]) != batch_dims:
      raise ValueError('frames and num_frames have different batch_dims: '
                       f'{tuple(frames.shape[:-2])} vs {batch_dims}')
    if tuple(labels.shape[:-1]) != batch_dims:
      raise ValueError('labels and num_frames have different batch_dims: '
                       f'{tuple(labels.shape[:-1])} vs {batch_dims}')
    if tuple(num_labels.shape) != batch_dims:
      raise ValueError('num_labels and num_frames have different batch_dims: '
                       f'{tuple(num_labels.shape)} vs {batch_dims}')
    W, nf, batch_dims, B, _, _, _ = self._prepare(cache, frames, num_frames)
    lab = torch.as_tensor(labels).reshape(B, -1).to(device=W.device, dtype=torch.int32).contiguous()
    nl = _lengths(num_labels, B, W.device)
    T_, U_ = W.shape[1], lab.shape[-1]
    lv = torch.as_tensor(lexical_values)
    if tuple(lv.shape) != (*batch_dims, T_, U_):
      raise ValueError(f'lexical_values should have the shape {(*batch_dims, T_, U_)}, but got '
                       f'{tuple(lv.shape)}')
    if blank_values is None:
      bv = torch.zeros([B, T_, U_ + 1], dtype=torch.float32, device=W.device)
    else:
      bv = torch.as_tensor(blank_values)
      if tuple(bv.shape) != (*batch_dims, T_, U_ + 1):
        raise ValueError(f'blank_values should have the shape {(*batch_dims, T_, U_ + 1)}, but '
                         f'got {tuple(bv.shape)}')
    lv = lv.to(W.device).reshape(B, T_, U_)
    bv = bv.to(W.device).reshape(B, T_, U_ + 1)
    if W.device.type == 'cpu':
      out = cpu.align_expectation(W, nf, lab, nl.long(), self.context, self.alignment, lv, bv)
    else:
      graph = self._graph(W.device)
      if _native.table_align_expectation_supported(graph, W, lab):
        out = _AlignExpectFn.apply(W, lv, bv, nf, lab, nl, graph)
      else:
        # the restatement on the device: the walk reads the graph's device copy
        # of the next-state table, nothing visits the host
        out = cpu.align_expectation(W.float(), nf.long(), lab, nl.long(),
                                    contexts.NextStateTable(graph.table), self.alignment, lv, bv)
    expected, log_prob = out
    return (self._home(expected.float().reshape(batch_dims), frames),
            self._home(log_prob.float().reshape(batch_dims), frames))

  def sample(self, frames: torch.Tensor, num_frames: torch.Tensor, num_samples: int, seed: int,
             cache: Optional[T] = None):
    """Alignment paths drawn from the lattice posterior p(pi) = exp(w(pi)) / Z,
    Z the normaliser of `forward` (not in the reference): Gumbel-max on
    Philox4x32-10 keyed by `seed`, walked backwards over the Log forward's
    alpha -- the definition in include/lt_sample.h, so the same seed gives
    the same paths on every device, and samples 0..S-1 do not depend on how
    many more the call draws. FrameDependent with any context that has a
    next-state table; FrameLabelDependent raises NotImplementedError.

    Returns (alignment_labels [batch..., S, T] int64, path_weights
    [batch..., S], log_z [batch...]): the true label y of the arc taken on
    each frame (0 = blank, 0 on padding frames) and the sum of the path's arc
    weights, so log p(pi) = path_weights - log_z. num_frames = 0 gives the
    empty path (weight 0); an utterance whose log_z is not finite is
    unsampled: labels all 0, weight -inf. No gradient flows through samples.
    """
    if not isinstance(self.alignment, alignments.FrameDependent):
      raise NotImplementedError('sample implements FrameDependent alignments, got '
                                f'{type(self.alignment).__name__}')
    S = int(num_samples)
    if S < 1:
      raise ValueError(f'num_samples should be >= 1, but got {num_samples}')
    W, nf, batch_dims, B, V, n, _ = self._prepare(cache, frames, num_frames)
    with torch.no_grad():
      W = W.detach()
      if W.device.type == 'cpu':
        labels, weights, log_z = cpu.sample(W, nf, self.context, S, seed)
      else:
        graph = self._graph(W.device)
        if self._table_path():
          log_z, alpha = _native.table_forward(graph, W, nf, _native.SEMIRING_LOG)
        else:
          log_z, alpha = _native.den_forward(W, nf, V, n, _native.SEMIRING_LOG)
        labels, weights = _native.table_sample(graph, W, nf, log_z, alpha, S, seed)
    T = W.shape[1]
    return (self._home(labels.reshape(*batch_dims, S, T), frames),
            self._home(weights.reshape(*batch_dims, S), frames),
            self._home(log_z.reshape(batch_dims), frames))

  def beam_search(self, frames: torch.Tensor, num_frames: torch.Tensor, beam_size: int,
                  semiring=semirings.Log, cache: Optional[T] = None):
    """The beam_size best label sequences with their scores (not in the
    reference): frame-synchronous beam search over label prefixes, the
    definition in include/lt_beam.h. A hypothesis is a label prefix; on each
    frame it stays (the blank arc) or grows by one label, a prefix reached
    both ways -- by staying, and as its parent's extension -- is one
    hypothesis whose two scores are (+)-summed, and the beam_size best
    candidates (larger score first, ties to the lower slot, then the lower
    label) make the next beam. With semirings.Log a score is the log of the
    summed weight of the sequence's alignments that the beam kept: at most
    _string_forward of the sequence, equal to it when nothing was pruned.
    With semirings.MaxTropical it is the best kept alignment's weight.
    Neither is normalised: subtract _forward's log_z for a log-probability.
    shortest_path returns the best alignment; this returns the best label
    sequences, which need not contain that alignment's.

    Returns (labels [batch..., K, T] int64, num_labels [batch..., K] int64,
    scores [batch..., K] fp32), best first: a sequence's labels at the front
    of its row, 0 after them; a slot the search could not fill (fewer than K
    candidates of finite score) holds all 0 / 0 / -inf; num_frames = 0 gives
    the empty sequence with score 0. No gradient flows through any of them.
    `labels` with `num_frames` goes straight into last_torch_amd.edit_distance
    as hypotheses: the zeros read as blanks. FrameDependent with any context
    that has a next-state table; FrameLabelDependent raises
    NotImplementedError. ROCm tensors run lt_table_beam_search (one launch);
    past its range (beam_size > 64, V > 1023) and on the host, the same
    definition in torch ops (cpu.beam_search).
    """
    if not isinstance(self.alignment, alignments.FrameDependent):
      raise NotImplementedError('beam_search implements FrameDependent alignments, got '
                                f'{type(self.alignment).__name__}')
    K = int(beam_size)
    if K < 1:
      raise ValueError(f'beam_size should be >= 1, but got {beam_size}')
    if getattr(semiring, 'name', None) not in ('Log', 'MaxTropical'):
      raise NotImplementedError(f'beam_search supports Log and MaxTropical, got {semiring!r}')
    W, nf, batch_dims, B, _, _, _ = self._prepare(cache, frames, num_frames)
    with torch.no_grad():
      W = W.detach()
      if W.device.type == 'cpu':
        labels, num_labels, scores = cpu.beam_search(W, nf, self.context, K, semiring)
      else:
        graph = self._graph(W.device)
        if _native.table_beam_search_supported(graph, W, K):
          labels, num_labels, scores = _native.table_beam_search(graph, W, nf, K,
                                                                 _semiring_id(semiring))
        else:
          labels, num_labels, scores = cpu.beam_search(
              W, nf, contexts.NextStateTable(graph.table), K, semiring)
    Tn = W.shape[1]
    return (self._home(labels.reshape(*batch_dims, K, Tn), frames),
            self._home(num_labels.long().reshape(*batch_dims, K), frames),
            self._home(scores.reshape(*batch_dims, K), frames))

  def _path_weights(self, W, nf, paths):
    """path weights [B, S] of paths [B, S, T] over prepared W / nf,
    differentiable w.r.t. W."""
    if W.device.type == 'cuda':
      graph = self._graph(W.device)
      if _native.table_path_score_supported(graph, W, paths.shape[1]):
        return _PathScoreFn.apply(W, nf, paths.contiguous(), graph)
      return cpu.path_weights(W, nf, paths, contexts.NextStateTable(graph.table))[0]
    return cpu.path_weights(W, nf, paths, self.context)[0]

  def path_weights(self, frames: torch.Tensor, num_frames: torch.Tensor,
                   alignment_labels: torch.Tensor, cache: Optional[T] = None) -> torch.Tensor:
    """The weights [batch..., S] of given alignment paths (not in the
    reference): alignment_labels [batch..., S, T] holds the true label y of
    the arc each path takes on each frame (0 = blank), the layout `sample`
    returns -- and what `align` and shortest_path(label_convention='true')
    return on FrameDependent, with an S axis added. The definition is
    include/lt_paths.h: a path walks the context's next-state table from the
    start state, and its weight is the fp32 sum of its arc weights added from
    the last live frame to the first, so the paths `sample` returned score to
    its path_weights bit for bit. Labels on padding frames are ignored; a
    live label outside [0, V] gives weight -inf and no gradient; num_frames
    = 0 gives 0.

    Differentiable w.r.t. the weight function: the gradient of a path's
    weight is the indicator of its arcs. FrameDependent with any context that
    has a next-state table; FrameLabelDependent raises NotImplementedError.
    """
    if not isinstance(self.alignment, alignments.FrameDependent):
      raise NotImplementedError('path_weights implements FrameDependent alignments, got '
                                f'{type(self.alignment).__name__}')
    W, nf, batch_dims, B, _, _, _ = self._prepare(cache, frames, num_frames)
    paths = torch.as_tensor(alignment_labels)
    Tn = W.shape[1]
    if (paths.ndim != len(batch_dims) + 2 or tuple(paths.shape[:-2]) != batch_dims or
        paths.shape[-1] != Tn):
      raise ValueError(f'alignment_labels should be [batch..., S, {Tn}] with batch dims '
                       f'{batch_dims}, got {tuple(paths.shape)}')
    S = paths.shape[-2]
    if S < 1:
      raise ValueError('alignment_labels holds no path (S = 0)')
    paths = paths.to(device=W.device, dtype=torch.int64).reshape(B, S, Tn)
    weights = self._path_weights(W, nf, paths)
    return self._home(weights.reshape(*batch_dims, S), frames)

  def sampled_risk(self, frames: torch.Tensor, num_frames: torch.Tensor, labels: torch.Tensor,
                   num_labels: torch.Tensor, num_samples: int, seed: int,
                   cost_fn: Optional[Callable[[torch.Tensor, torch.Tensor], torch.Tensor]] = None,
                   cache: Optional[T] = None):
    """Minimum-risk (expected-cost) training from sampled paths (not in the
    reference): the risk R = sum_pi p(pi) c(pi) of a path cost c under the
    lattice posterior p(pi) = exp(w(pi)) / Z, estimated from num_samples paths
    drawn exactly as `sample` draws them (same seed contract).

    Returns (risk [batch...], costs [batch..., S], alignment_labels
    [batch..., S, T]). The default cost is the edit distance
    (last_torch_amd.edit_distance) of each path's labels to labels /
    num_labels, as float32; cost_fn(alignment_labels, num_frames) ->
    [batch..., S] replaces it. risk = costs.mean(-1) in value. An unsampled
    utterance (log_z not finite) has risk 0, costs 0 and a zero gradient.

    Gradient (into the weight function only; none flows into costs or
    labels). dR/dw_a = Cov_p(c, 1[a in pi]):
      * S >= 2: the leave-one-out score-function estimator
        1/(S-1) sum_s (c_s - mean c) 1[a in pi_s], the unbiased sample
        covariance, as sum_s adv_s * path_weight_s with adv detached. The
        advantages sum to zero, so the log Z term cancels exactly and no
        marginal pass runs: the backward is one scatter of S*T scalars.
      * S = 1 (no baseline): c * (path_weight - log_z), whose gradient
        c * (1[a in pi] - marginal_a) runs the Log backward of `_forward`.
    One arc_weights call. FrameDependent with any context that has a
    next-state table; FrameLabelDependent raises NotImplementedError.
    """
    if not isinstance(self.alignment, alignments.FrameDependent):
      raise NotImplementedError('sampled_risk implements FrameDependent alignments, got '
                                f'{type(self.alignment).__name__}')
    S = int(num_samples)
    if S < 1:
      raise ValueError(f'num_samples should be >= 1, but got {num_samples}')
    W, nf, batch_dims, B, V, n, _ = self._prepare(cache, frames, num_frames)
    Tn = W.shape[1]
    want_grad = torch.is_grad_enabled() and W.requires_grad
    # log Z and alpha: in the graph only where the estimator needs d log Z
    with torch.set_grad_enabled(want_grad and S == 1):
      if W.device.type == 'cpu':
        log_z, alpha = cpu.den_forward(W, nf, self.context, self.alignment, semirings.Log)
      elif self._table_path():
        log_z, alpha = _TableDenFn.apply(W, nf, self._graph(W.device), _native.SEMIRING_LOG)
      else:
        log_z, alpha = _DenFn.apply(W, nf, V, n, _native.SEMIRING_LOG, None)
    with torch.no_grad():
      if W.device.type == 'cpu':
        paths = cpu.sample(W.detach(), nf, self.context, S, seed, log_z=log_z.detach(),
                           alpha=alpha.detach())[0]
      else:
        paths = _native.table_sample(self._graph(W.device), W.detach(), nf, log_z.detach(),
                                     alpha.detach(), S, seed)[0]
      shaped = paths.reshape(*batch_dims, S, Tn)
      if cost_fn is None:
        costs = risk_lib.edit_distance(shaped, nf.reshape(batch_dims), labels, num_labels)
      else:
        costs = cost_fn(self._home(shaped, frames), num_frames)
      costs = torch.as_tensor(costs).detach().to(device=W.device, dtype=torch.float32)
      if tuple(costs.shape) != (*batch_dims, S):
        raise ValueError(f'costs should be {(*batch_dims, S)}, got {tuple(costs.shape)}')
      sampled = torch.isfinite(log_z.detach())[:, None]                     # [B, 1]
      costs = torch.where(sampled, costs.reshape(B, S), torch.zeros([], device=W.device))
      risk = costs.mean(dim=-1)
      adv = costs if S == 1 else (costs - risk[:, None]) / (S - 1)
    if want_grad:
      zero = torch.zeros([], device=W.device)
      score = torch.where(sampled, self._path_weights(W, nf, paths), zero)
      if S == 1:
        score = score - torch.where(sampled, log_z.float()[:, None], zero)
      surrogate = (adv * score).sum(dim=-1)
      risk = risk + (surrogate - surrogate.detach())
    return (self._home(risk.reshape(batch_dims), frames),
            self._home(costs.reshape(*batch_dims, S), frames),
            self._home(shaped, frames))

  @staticmethod
  def _align_dense(graph, W, nf, lab, nl):
    """align through the dense one-hot string gradient
    (lt_table_num_backward in MaxTropical, [B, T, C, V+1]) and a torch
    compaction: a frame's lexical arcs are the next `count` string positions,
    count = the sum of its lexical gradients."""
    num, dW = _native.table_num_backward(graph, W, nf, lab, nl, _native.SEMIRING_MAX)
    B, T = W.shape[:2]
    U = lab.shape[-1]
    A = graph.num_alignment_states()
    aligned = num > -torch.inf
    count = dW[..., 1:].float().sum(dim=(2, 3)).round().long() * aligned[:, None]  # [B, T]
    end = torch.cumsum(count, dim=1)
    start = end - count
    pos = torch.arange(U, device=W.device).expand(B, U).contiguous()
    frame = torch.searchsorted(end.contiguous(), pos, right=True)
    label_frames = torch.where(frame < T, frame, torch.full_like(frame, -1))
    true = torch.where((lab >= 1) & (lab <= graph.V), lab, torch.zeros_like(lab)).long()
    slot = torch.arange(A, device=W.device)
    idx = start[:, :, None] + slot                                      # [B, T, A]
    padded = torch.cat([true, true.new_zeros([B, 1])], dim=1)
    picked = torch.gather(padded, 1, idx.clamp(max=U).reshape(B, T * A)).reshape(B, T, A)
    alignment_labels = torch.where(slot < count[:, :, None], picked, torch.zeros_like(picked))
    return alignment_labels.reshape(B, T * A), label_frames, num

  def _string_forward(self, cache: T, frames: torch.Tensor, num_frames: torch.Tensor,
                      labels: torch.Tensor, num_labels: torch.Tensor,
                      semiring: semirings.Semiring) -> torch.Tensor:
    """Shortest distance on the lattice intersected with the label string
    (lattices.py:250-377)."""
    batch_dims = tuple(num_frames.shape)
    if tuple(frames.shape[:-2]) != batch_dims:
      raise ValueError('frames and num_frames have different batch_dims: '
                       f'{tuple(frames.shape[:-2])} vs {batch_dims}')
    if tuple(labels.shape[:-1]) != batch_dims:
      raise ValueError('labels and num_frames have different batch_dims: '
                       f'{tuple(labels.shape[:-1])} vs {batch_dims}')
    if tuple(num_labels.shape) != batch_dims:
      raise ValueError('num_labels and num_frames have different batch_dims: '
                       f'{tuple(num_labels.shape)} vs {batch_dims}')
    sid = _semiring_id(semiring)
    W, nf, batch_dims, B, V, n, _ = self._prepare(cache, frames, num_frames)
    lab = torch.as_tensor(labels).reshape(B, -1).to(device=W.device, dtype=torch.int32)
    nl = _lengths(num_labels, B, W.device)
    if W.device.type == 'cpu':
      num = cpu.num_forward(W, nf, lab, nl.long(), self.context, self.alignment, semiring)
    elif self._table_path():
      num = _TableNumFn.apply(W, nf, lab.contiguous(), nl, self._graph(W.device), sid)
    else:
      # MaxTropical / Real gradients run on the general string-gradient kernel
      # over FullNGram.next_state_table(): its graph is built only when a
      # gradient can be asked for, and its LDS rule is checked here, before
      # the forward, rather than mid-backward
      graph = None
      if sid != _native.SEMIRING_LOG and torch.is_grad_enabled() and W.requires_grad:
        graph = self._graph(W.device)
        _native.table_num_backward_check(graph, W, lab, sid)
      num = _NumFn.apply(W, nf, lab.contiguous(), nl, V, n, sid, graph)
    return self._home(num.reshape(batch_dims), frames)

  def _forward(self, cache: T, frames: torch.Tensor, num_frames: torch.Tensor,
               semiring: semirings.Semiring,
               blank_mask: Optional[Sequence[torch.Tensor]] = None,
               lexical_mask: Optional[Sequence[torch.Tensor]] = None):
    """Shortest distance and alpha_0..T-1 (lattices.py:379-496).

    Masks are added to the arc weights (lattices.py:450-453), so their
    gradients are the arc marginals (Log) or the best-path indicator
    (MaxTropical) -- per utterance, without the batch aliasing of D6.
    """
    if semiring is semirings.LogLogExpectation and blank_mask is None and lexical_mask is None:
      return self._forward_expectation(cache, frames, num_frames)
    for name, mask in (('blank_mask', blank_mask), ('lexical_mask', lexical_mask)):
      if mask is not None and len(mask) != self.alignment.num_states():
        raise ValueError(f'The length of {name} should be equal to '
                         f'{self.alignment.num_states()} (the number of alignment states), '
                         f'but is {len(mask)}')
    sid = _semiring_id(semiring)
    batch_dims = tuple(num_frames.shape)
    if tuple(frames.shape[:-2]) != batch_dims:
      raise ValueError('frames and num_frames have different batch_dims: '
                       f'{tuple(frames.shape[:-2])} vs {batch_dims}')
    table = self._table_path()
    V, n = self._ngram() if not table else (None, None)
    if table:
      # alignment-state-invariant weights (lattices.py:444-447): one mask
      # for every alignment state
      for mask in (blank_mask, lexical_mask):
        if mask is not None and any(m is not mask[0] and not torch.equal(m, mask[0])
                                    for m in mask[1:]):
          raise NotImplementedError('per-alignment-state masks differ: the kernels use '
                                    'alignment-state-invariant weights')
    if cache is None:
      cache = self.weight_fn_cacher()
    W = self.arc_weights(cache, frames)
    if blank_mask is not None:
      W = torch.cat([W[..., :1] + blank_mask[0].to(W.device)[..., None], W[..., 1:]], dim=-1)
    if lexical_mask is not None:
      W = torch.cat([W[..., :1], W[..., 1:] + lexical_mask[0].to(W.device)], dim=-1)
    B = 1
    for d in batch_dims:
      B *= d
    dev = _compute_device(W, frames, num_frames)
    nf = _lengths(num_frames, B, dev)
    if dev.type == 'cpu':
      dist, alpha = cpu.den_forward(W.reshape(B, *W.shape[-3:]).float(), nf.long(), self.context,
                                    self.alignment, semiring)
      C = alpha.shape[-1]
      return (dist.reshape(batch_dims),
              alpha.reshape(*batch_dims, frames.shape[-2], C))
    Wk = _kernel_weights(W.to(dev).reshape(B, *W.shape[-3:]))
    if table:
      dist, alpha = _TableDenFn.apply(Wk, nf, self._graph(Wk.device), sid)
    else:
      graph = self._graph(Wk.device) if sid == _native.SEMIRING_REAL else None
      dist, alpha = _DenFn.apply(Wk, nf, V, n, sid, graph)
    C = alpha.shape[-1]
    return (self._home(dist.reshape(batch_dims), frames),
            self._home(alpha.reshape(*batch_dims, frames.shape[-2], C), frames))

  def _expectation(self, cache, frames, num_frames):
    """(log Z, sum over arcs of m(arc) * w(arc)) per utterance, m the arc
    marginals (the gradient of log Z: the den backward kernel on a ROCm
    device, autograd through cpu.py on the CPU). FullNGram x FrameDependent."""
    W, nf, batch_dims, B, V, n, _ = self._prepare(cache, frames, num_frames)
    with torch.enable_grad():
      Wd = W.detach().requires_grad_(True)
      if Wd.device.type == 'cpu':
        log_z, _ = cpu.den_forward(Wd, nf, self.context, self.alignment, semirings.Log)
      elif self._table_path():
        log_z, _ = _TableDenFn.apply(Wd, nf, self._graph(Wd.device), _native.SEMIRING_LOG)
      else:
        log_z, _ = _DenFn.apply(Wd, nf, V, n, _semiring_id(semirings.Log))
      (m,) = torch.autograd.grad(log_z.sum(), Wd)
    # arcs of zero weight (w = -inf) carry m = 0 and contribute nothing
    mw = torch.where(m > 0, m * Wd.detach().float(), torch.zeros_like(m)).sum(dim=(-3, -2, -1))
    return log_z.detach(), mw, batch_dims

  def _forward_expectation(self, cache, frames, num_frames):
    """_forward under semirings.LogLogExpectation (semirings.py:405-484).
    The lattice's arc weights are single tensors, so every arc carries the
    expectation pair weighted(w, -w): the value -w, the convention of the
    reference's entropy test (tests/semirings_test.py:305-312). The shortest
    distance is then (log Z, log Z + log E_p[-w_path]) by the forward-backward
    identity (the x component sums Z m(arc) v(arc) over arcs). Returns
    ((log_z, log_sum), None): there is no per-frame alpha of a pair."""
    log_z, mw, batch_dims = self._expectation(cache, frames, num_frames)
    log_sum = log_z + torch.log(-mw)
    return ((self._home(log_z.reshape(batch_dims), frames),
             self._home(log_sum.reshape(batch_dims), frames)), None)

  def _expect(self, W, values, nf):
    """(E [B], log_z [B]) for flattened arc weights and values on W's device:
    cpu.expectation (plain autograd) or _ExpectFn (lt_table_expectation)."""
    if W.device.type == 'cpu':
      return cpu.expectation(W, values.to(W.device), nf, self.context)
    return _ExpectFn.apply(W, values.to(W.device), nf, self._graph(W.device))

  def expectation(self, frames: torch.Tensor, num_frames: torch.Tensor, values: torch.Tensor,
                  cache: Optional[T] = None):
    """Posterior mean of an arc-additive path value (not in the reference;
    the definition is in include/lt_expect.h): with p(pi) = exp(w(pi)) / Z
    over the alignment paths of `forward`'s denominator lattice,
    expected = sum_pi p(pi) sum_{a in pi} values[a]. `values` has the layout
    of the arc weights, [batch..., T, C, V+1] ([..., 0] the blank arc of a
    state, [..., y] its label-y arc), and may have any sign.

    Returns (expected [batch...], log_z [batch...]). Both are differentiable
    w.r.t. the weight function through the arc weights, and `expected` also
    w.r.t. `values`: d expected / d values is the arc marginal m_a and
    d expected / d w_a = m_a (E[v | a] - expected). On ROCm tensors the
    gradients come from one lt_table_expectation call with the forward and are
    not twice differentiable; on CPU tensors they are plain autograd.
    An arc of weight -inf contributes nothing and its value is ignored (NaN
    or inf there is harmless); num_frames = 0 gives (0, 0); an utterance whose
    log_z is not finite gives expected = 0 and zero gradients. FrameDependent
    with any context that has a next-state table; FrameLabelDependent raises
    NotImplementedError."""
    if not isinstance(self.alignment, alignments.FrameDependent):
      raise NotImplementedError('expectation implements FrameDependent alignments, got '
                                f'{type(self.alignment).__name__}')
    W, nf, batch_dims, B, _, _, _ = self._prepare(cache, frames, num_frames)
    values = torch.as_tensor(values)
    if tuple(values.shape) != (*batch_dims, *W.shape[1:]):
      raise ValueError(f'values should have the shape of the arc weights '
                       f'{(*batch_dims, *W.shape[1:])}, but got {tuple(values.shape)}')
    expected, log_z = self._expect(W, values.reshape(W.shape), nf)
    return (self._home(expected.reshape(batch_dims), frames),
            self._home(log_z.reshape(batch_dims), frames))

  def entropy(self, frames: torch.Tensor, num_frames: torch.Tensor,
              cache: Optional[T] = None, differentiable: bool = False) -> torch.Tensor:
    """Entropy (nats) of the alignment-path distribution p(path) = exp(w_path)
    / Z of every utterance: H = log Z - E_p[w_path], the lattice entropy the
    LogLogExpectation semiring computes (tests/semirings_test.py:305-312:
    entropy = log_z + exp(log_sum - log_z)), here for weights of any sign.
    Values only (no gradient) by default. differentiable=True returns H with
    a graph w.r.t. the weight function (entropy regularisation): one
    arc_weights call, then `expectation`'s function on (W, -W); FrameDependent
    only, and on ROCm tensors not twice differentiable."""
    if differentiable:
      if not isinstance(self.alignment, alignments.FrameDependent):
        raise NotImplementedError('entropy(differentiable=True) implements FrameDependent '
                                  f'alignments, got {type(self.alignment).__name__}')
      W, nf, batch_dims, _, _, _, _ = self._prepare(cache, frames, num_frames)
      neg_w, log_z = self._expect(W, -W.float(), nf)  # E_p[-w_path]
      return self._home((log_z + neg_w).reshape(batch_dims), frames)
    log_z, mw, batch_dims = self._expectation(cache, frames, num_frames)
    return self._home((log_z - mw).reshape(batch_dims), frames)

  def _forward_backward(self, cache: T, frames: torch.Tensor, num_frames: torch.Tensor):
    """log_z with gradients from the backward algorithm (lattices.py:498-642;
    the reference's backward raises, D3). Returns (log_z, alpha_0..T-1)."""
    return self._forward(cache, frames, num_frames, semirings.Log)

  class BackwardStepCallback(Protocol):
    """Callback of the backward algorithm loop (lattices.py:644-684)."""

    def __call__(self, weight_vjp_fn, carry, blank_marginal: torch.Tensor,
                 lexical_marginals: torch.Tensor) -> tuple[Any, Any]:
      raise NotImplementedError

  def _backward(self, cache: T, frames: torch.Tensor, num_frames: torch.Tensor,
                log_z: torch.Tensor, alpha_0_to_T_minus_1: torch.Tensor,
                init_callback_carry: Any, callback: BackwardStepCallback):
    """Arc marginals by the backward algorithm (lattices.py:686-799).

    The marginals of every frame come from one ``lt_den_backward`` launch;
    the callback then runs frame by frame from T-1 down to 0 (the reference
    iterates in the wrong direction, D4) with ``weight_vjp_fn`` for that
    frame. Outputs are stacked in time order along the frame axis.
    """
    batch_dims = tuple(num_frames.shape)
    if tuple(frames.shape[:-2]) != batch_dims:
      raise ValueError('frames and num_frames have different batch_dims: '
                       f'{tuple(frames.shape[:-2])} vs {batch_dims}')
    if tuple(log_z.shape) != batch_dims:
      raise ValueError('log_z and num_frames have different batch_dims: '
                       f'{tuple(log_z.shape)} vs {batch_dims}')
    if tuple(alpha_0_to_T_minus_1.shape[:-2]) != batch_dims:
      raise ValueError('alpha_0_to_T_minus_1 and num_frames have different '
                       f'batch_dims: {tuple(alpha_0_to_T_minus_1.shape[:-2])} vs {batch_dims}')
    with torch.no_grad():
      W = self.arc_weights(cache, frames)
      B = 1
      for d in batch_dims:
        B *= d
      dev = _compute_device(W, frames, num_frames)
      nf = _lengths(num_frames, B, dev)
    if dev.type == 'cpu':
      # arc marginals = d log_z / dW (the reference's backward algorithm
      # computes the same quantities frame by frame)
      with torch.enable_grad():
        Wd = W.detach().reshape(B, *W.shape[-3:]).float().requires_grad_(True)
        dist, _ = cpu.den_forward(Wd, nf.long(), self.context, self.alignment, semirings.Log)
        (marg,) = torch.autograd.grad(dist.sum(), Wd)
      marg = marg.reshape(*batch_dims, *marg.shape[1:])
    else:
      with torch.no_grad():
        Wk = _kernel_weights(W.to(dev).reshape(B, *W.shape[-3:]))
        lz = log_z.detach().reshape(B).to(dev, torch.float32).contiguous()
        al = alpha_0_to_T_minus_1.detach().reshape(B, Wk.shape[1], -1).to(dev, torch.float32)
        if self._table_path():
          # any next-state table, FrameDependent or FrameLabelDependent
          # (self.alignment.backward, lattices.py:764)
          marg = _native.table_den_backward(self._graph(dev), Wk, nf, _native.SEMIRING_LOG, lz,
                                            al.contiguous()).float()
        else:
          V, n = self._ngram()
          marg = _native.den_backward(Wk, nf, lz, al.contiguous(), None, V, n).float()
        marg = self._home(marg.reshape(*batch_dims, *marg.shape[1:]), frames)
    tdim = len(batch_dims)
    carry, outs = init_callback_carry, []
    # weight_vjp_fn(cotangent) -> (d cache, d frame); a cache that is not a
    # tree of tensors (NullCacher: None) is held fixed and gets None
    leaves = torch.utils._pytree.tree_leaves(cache)
    cache_is_tensor = cache is not None and all(isinstance(x, torch.Tensor) for x in leaves)

    def frame_vjp(frame):
      if cache_is_tensor:
        return torch.func.vjp(lambda c, f: self.weight_fn(c, f), cache, frame)[1]
      fn = torch.func.vjp(lambda f: self.weight_fn(cache, f), frame)[1]
      return lambda ct: (None, *fn(ct))

    for t in reversed(range(frames.shape[-2])):
      frame = frames.select(tdim, t)
      vjp_fn = frame_vjp(frame)
      m = marg.select(tdim, t)
      carry, out = callback(weight_vjp_fn=vjp_fn, carry=carry, blank_marginal=m[..., 0],
                            lexical_marginals=m[..., 1:])
      outs.append(out)
    outs.reverse()
    stacked = torch.utils._pytree.tree_map(lambda *xs: torch.stack(xs, dim=tdim), *outs) \
        if outs else None
    return carry, stacked
