"""The dummy lt_graph of the CPU ABI tests: every array points at one host
buffer, which the validation code under test never dereferences."""
from last_torch_amd import _native


def dummy_graph(p, K=0, C=33, V=32):
  """Graph of C states, V labels and K expansions whose arrays are all p (a
  ctypes.c_void_p)."""
  return _native.Graph(C, V, K, p.value, p.value, p.value)
