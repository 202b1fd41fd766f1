"""lt_table_align_long (include/lt_align_long.h) without a GPU: the header, the
exports and the binding agree, and the host validation's error codes, which
come back before any device work (as test_align_cpu.py checks lt_table_align's).
"""
import ctypes
import os
import re

from last_torch_amd import _native
from abi_graph import dummy_graph
from test_align_cpu import HEADER, _define

INCLUDE = os.path.dirname(HEADER)


def test_library_exports_what_lt_align_long_h_declares():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(INCLUDE, 'lt_align_long.h')).read(), flags=re.S)
  declared = sorted(set(re.findall(r'\b(lt_[a-z_]+)\s*\(', src)))
  assert declared == sorted(_native.EXPORTED_ALIGN_LONG) and len(declared) == 2
  for name in declared:
    assert hasattr(_native.lib(), name) and name in _native._SIG
    assert name not in _native.EXPORTED
  assert '#include "lt_align_long.h"' in open(os.path.join(INCLUDE, 'lt_align.h')).read()


def test_align_long_host_validation_error_codes():
  lib = _native.lib()
  EINVAL, EUNSUPPORTED = _define('LT_EINVAL'), _define('LT_EUNSUPPORTED')
  null = ctypes.c_void_p(0)
  # host arrays stand in for the device pointers: nothing below dereferences them
  buf = (ctypes.c_int64 * 64)()
  p = ctypes.c_void_p(ctypes.addressof(buf))
  nbytes = ctypes.c_size_t(7)
  TP = _native.TableProblem

  def query(g, pb):
    return lib.lt_table_align_long_workspace_bytes(ctypes.byref(g), ctypes.byref(pb),
                                                   ctypes.byref(nbytes))

  def call(g, pb, W=p, out=p, w=p, ws=p, size=1 << 40):
    return lib.lt_table_align_long(ctypes.byref(g), ctypes.byref(pb), W, p, p, p, out, p, w, ws,
                                   size, null)

  ok = TP(batch=2, max_frames=4, max_labels=300, weight_dtype=0)
  for g, pb in [(dummy_graph(p), TP(batch=2, max_frames=4, max_labels=255, weight_dtype=0)),
                (dummy_graph(p), TP(batch=2, max_frames=4, max_labels=4096, weight_dtype=0)),
                (dummy_graph(p, K=1), ok)]:
    assert query(g, pb) == EUNSUPPORTED
    assert b'lt_table_align_long' in lib.lt_last_error()
    assert call(g, pb) == EUNSUPPORTED
    assert b'lt_table_align_long' in lib.lt_last_error()
  assert call(dummy_graph(p), ok, W=null) == EINVAL
  assert b'null pointer' in lib.lt_last_error()
  assert call(dummy_graph(p), ok, out=ctypes.c_void_p(p.value + 4)) == EINVAL
  assert b'misaligned' in lib.lt_last_error()
  assert call(dummy_graph(p), TP(batch=2, max_frames=4, max_labels=300, weight_dtype=5)) == EINVAL
  assert call(dummy_graph(p), ok, ws=null, size=0) == EINVAL
  assert b'workspace' in lib.lt_last_error()
  assert call(dummy_graph(p), TP(batch=0, max_frames=4, max_labels=4095, weight_dtype=0),
              W=null, w=null, ws=null, size=0) == 0
  # the header's formula: batch * max_frames * 32 * NW bytes, rounded up to 256
  for B, T, U in [(3, 5, 256), (64, 4200, 4095), (1, 1, 1024)]:
    assert query(dummy_graph(p), TP(batch=B, max_frames=T, max_labels=U, weight_dtype=1)) == 0
    NW = (U + 256) // 256
    assert nbytes.value == (B * T * 32 * NW + 255) // 256 * 256
