"""A test-only allocator shim for the ctypes bindings -- TEST INFRASTRUCTURE.

``last_torch_amd._native`` and ``_native_cpu`` allocate every output and every
workspace with ``torch.empty`` / ``torch.empty_like``, reached through their
module attribute ``torch``. The two context managers here swap that attribute
for a proxy that forwards everything else to the real ``torch``:

  * ``poisoned(mod)``: every allocation is filled with 0xFF bytes (NaN in fp32
    and bf16, -1 in int32 / int64, 255 in uint8) before the binding sees it,
    so an element the kernel never stores cannot pass for a promised zero.
  * ``stale(mod)``: ``record(fn, ...)`` runs a call and keeps every tensor the
    allocator handed out, in order; ``replay(fn, ...)`` hands the same tensors
    back, in the same order, to a second call of the same shape on other data.
    The second call finds every output and workspace byte as a finished call
    on another problem left it (its values, its flags, its tags). It returns
    the SAME tensors: clone() whatever of the first call is still needed.

Nothing here is used by the product path.
"""
import contextlib

import torch as _torch

POISON_BYTE = 0xFF


def poison_(t):
  """Fills `t` (any dtype, contiguous) with POISON_BYTE bytes, in place."""
  if t.numel():
    t.reshape(-1).view(_torch.uint8).fill_(POISON_BYTE)
  return t


class _TorchProxy:
  """`torch` with its own empty / empty_like; every other attribute is the
  real module's."""

  def __init__(self, empty, empty_like):
    self.empty = empty
    self.empty_like = empty_like

  def __getattr__(self, name):
    return getattr(_torch, name)


@contextlib.contextmanager
def _patched(mod, proxy):
  real = mod.torch
  assert real is _torch, f'{mod.__name__}.torch is already patched'
  mod.torch = proxy
  try:
    yield
  finally:
    mod.torch = real


@contextlib.contextmanager
def poisoned(mod):
  """Within the block, every torch.empty / torch.empty_like of `mod` returns
  0xFF bytes."""
  proxy = _TorchProxy(lambda *a, **k: poison_(_torch.empty(*a, **k)),
                      lambda *a, **k: poison_(_torch.empty_like(*a, **k)))
  with _patched(mod, proxy):
    yield


def _sig(t):
  return tuple(t.shape), t.dtype, t.device


class _Stale:
  """The record / replay pair of stale(mod)."""

  def __init__(self, mod):
    self._mod = mod
    self.tensors = []

  def record(self, fn, *args, **kwargs):
    """Runs fn(*args, **kwargs) and keeps every tensor it allocated."""
    assert not self.tensors, 'record() runs once per stale() block'

    def keep(t):
      self.tensors.append(t)
      return t

    proxy = _TorchProxy(lambda *a, **k: keep(_torch.empty(*a, **k)),
                        lambda *a, **k: keep(_torch.empty_like(*a, **k)))
    with _patched(self._mod, proxy):
      return fn(*args, **kwargs)

  def replay(self, fn, *args, **kwargs):
    """Runs fn(*args, **kwargs) on the recorded tensors: the i-th allocation
    gets the i-th recorded tensor as it stands, and must ask for its shape,
    dtype and device; the call must allocate exactly as many."""
    it = iter(self.tensors)
    handed = []

    def give(make, a, k):
      want = make(*a, **k)  # the request, for its shape / dtype / device
      t = next(it, None)
      assert t is not None, (f'replay: allocation {len(handed)} {_sig(want)} has no recorded '
                             f'counterpart ({len(self.tensors)} recorded)')
      assert _sig(t) == _sig(want), (f'replay: allocation {len(handed)} asks for {_sig(want)}, '
                                     f'recorded {_sig(t)}')
      handed.append(t)
      return t

    proxy = _TorchProxy(lambda *a, **k: give(_torch.empty, a, k),
                        lambda *a, **k: give(_torch.empty_like, a, k))
    with _patched(self._mod, proxy):
      out = fn(*args, **kwargs)
    assert len(handed) == len(self.tensors), (f'replay: {len(handed)} allocations, '
                                              f'{len(self.tensors)} recorded')
    return out


@contextlib.contextmanager
def stale(mod):
  """Yields the record / replay pair for `mod` (see the module docstring)."""
  s = _Stale(mod)
  try:
    yield s
  finally:
    s.tensors = []
