"""lt_table_align_posteriors_long's host validation (no GPU: nothing below
launches or dereferences a device pointer): its range, the documented
workspace size, the NULL and workspace rules, and that the library exports
what include/lt_posterior_long.h declares."""
import ctypes
import os
import re

from last_torch_amd import _native
from abi_graph import dummy_graph

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include')
OK, EINVAL, EUNSUPPORTED = 0, -1, -2  # LT_OK, LT_EINVAL, LT_EUNSUPPORTED (lt_lattice.h)


def test_library_exports_what_lt_posterior_long_h_declares():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(INCLUDE, 'lt_posterior_long.h')).read(),
               flags=re.S)
  declared = sorted(set(re.findall(r'\b(lt_[a-z_]+)\s*\(', src)))
  assert declared == sorted(_native.EXPORTED_POSTERIOR_LONG) and len(declared) == 2
  for name in declared:
    assert hasattr(_native.lib(), name) and name in _native._SIG
    assert name not in _native.EXPORTED
  assert '#include "lt_posterior_long.h"' in open(os.path.join(INCLUDE, 'lt_posterior.h')).read()


def test_long_align_posteriors_host_validation_error_codes():
  lib = _native.lib()
  null = ctypes.c_void_p(0)
  buf = (ctypes.c_int64 * 64)()  # stands in for the device pointers
  p = ctypes.c_void_p(ctypes.addressof(buf))
  TP = _native.TableProblem

  def call(g, pb, lp=p, ws=p, nbytes=1 << 40):
    return lib.lt_table_align_posteriors_long(ctypes.byref(g), ctypes.byref(pb), p, p, p, p, p, lp,
                                              ws, nbytes, null)

  def query(g, pb, nbytes):
    return lib.lt_table_align_posteriors_long_workspace_bytes(ctypes.byref(g), ctypes.byref(pb),
                                                              ctypes.byref(nbytes))

  nbytes = ctypes.c_size_t(7)
  for U in (255, 1024):  # 255 is lt_table_align_posteriors' own
    pb = TP(batch=2, max_frames=4, max_labels=U, weight_dtype=0)
    assert query(dummy_graph(p), pb, nbytes) == EUNSUPPORTED and call(dummy_graph(p), pb) == EUNSUPPORTED
  for K in (1, 2):
    pb = TP(batch=2, max_frames=4, max_labels=300, weight_dtype=0)
    assert query(dummy_graph(p, K=K), pb, nbytes) == EUNSUPPORTED
    assert call(dummy_graph(p, K=K), pb) == EUNSUPPORTED
  assert nbytes.value == 7  # a refused query writes nothing
  # the history: batch * max_frames * 256 NW * 8 bytes, rounded up to 256
  for U, NW in ((256, 2), (1023, 4)):
    pb = TP(batch=3, max_frames=5, max_labels=U, weight_dtype=1)
    assert query(dummy_graph(p), pb, nbytes) == OK
    assert nbytes.value == (3 * 5 * 256 * NW * 8 + 255) // 256 * 256
    assert call(dummy_graph(p), pb, lp=null) == EINVAL
    assert b'null pointer' in lib.lt_last_error()
    assert call(dummy_graph(p), pb, nbytes=nbytes.value - 1) == EINVAL
    assert b'workspace' in lib.lt_last_error()
