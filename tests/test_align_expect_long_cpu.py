"""Host validation of lt_table_align_expectation_long and
lt_table_string_scatter_long (no GPU: nothing below launches or dereferences a
device pointer): their range, the documented workspace size, the NULL and
workspace rules, and that the library exports what
include/lt_string_expect_long.h declares."""
import ctypes
import os
import re

from last_torch_amd import _native
from abi_graph import dummy_graph

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include')
OK, EINVAL, EUNSUPPORTED = 0, -1, -2  # LT_OK, LT_EINVAL, LT_EUNSUPPORTED (lt_lattice.h)


def test_library_exports_what_lt_string_expect_long_h_declares():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(INCLUDE, 'lt_string_expect_long.h')).read(),
               flags=re.S)
  declared = sorted(set(re.findall(r'\b(lt_[a-z_]+)\s*\(', src)))
  assert declared == sorted(_native.EXPORTED_ALIGN_EXPECT_LONG) and len(declared) == 3
  for name in declared:
    assert hasattr(_native.lib(), name) and name in _native._SIG
    assert name not in _native.EXPORTED
  short = open(os.path.join(INCLUDE, 'lt_string_expect.h')).read()
  assert '#include "lt_string_expect_long.h"' in short


def test_long_align_expectation_host_validation_error_codes():
  lib = _native.lib()
  null = ctypes.c_void_p(0)
  buf = (ctypes.c_int64 * 64)()  # stands in for the device pointers
  p = ctypes.c_void_p(ctypes.addressof(buf))
  odd = ctypes.c_void_p(p.value + 2)
  TP = _native.TableProblem

  def call(g, pb, E=p, lp=p, arrays=(p, p, p, p), ws=p, nbytes=1 << 40):
    return lib.lt_table_align_expectation_long(ctypes.byref(g), ctypes.byref(pb), p, p, p, p, p, p,
                                               E, lp, *arrays, ws, nbytes, null)

  def scatter(g, pb):
    return lib.lt_table_string_scatter_long(ctypes.byref(g), ctypes.byref(pb), p, p, p, p, p, p,
                                            null)

  def query(g, pb, nbytes):
    return lib.lt_table_align_expectation_long_workspace_bytes(ctypes.byref(g), ctypes.byref(pb),
                                                               ctypes.byref(nbytes))

  nbytes = ctypes.c_size_t(7)
  for U in (255, 1024):  # 255 is lt_table_align_expectation's own
    pb = TP(batch=2, max_frames=4, max_labels=U, weight_dtype=0)
    g = dummy_graph(p)
    assert query(g, pb, nbytes) == EUNSUPPORTED
    assert call(g, pb) == EUNSUPPORTED and scatter(g, pb) == EUNSUPPORTED
  for K in (1, 2):
    pb = TP(batch=2, max_frames=4, max_labels=300, weight_dtype=0)
    g = dummy_graph(p, K=K)
    assert query(g, pb, nbytes) == EUNSUPPORTED
    assert call(g, pb) == EUNSUPPORTED and scatter(g, pb) == EUNSUPPORTED
  assert nbytes.value == 7  # a refused query writes nothing
  # the history: batch * max_frames * 256 NW * 12 bytes, rounded up to 256
  for U, NW in ((256, 2), (1023, 4)):
    pb = TP(batch=3, max_frames=5, max_labels=U, weight_dtype=1)
    g = dummy_graph(p)
    assert query(g, pb, nbytes) == OK
    assert nbytes.value == (3 * 5 * 256 * NW * 12 + 255) // 256 * 256
    for kw in (dict(E=null), dict(lp=null)):
      assert call(g, pb, **kw) == EINVAL
      assert b'null pointer' in lib.lt_last_error()
    # a short or missing workspace is refused as soon as one array is requested ...
    for arrays in ((p, p, p, p), (null, null, null, p), (p, null, null, null)):
      assert call(g, pb, arrays=arrays, nbytes=nbytes.value - 1) == EINVAL
      assert b'workspace' in lib.lt_last_error()
      assert call(g, pb, arrays=arrays, ws=null, nbytes=0) == EINVAL
      assert b'workspace' in lib.lt_last_error()
    # ... and not looked at by the value-only call: its validation goes on past
    # the workspace rule to the alignment rule, which a 2-byte offset fails
    assert call(g, pb, E=odd, arrays=(null,) * 4, ws=null, nbytes=0) == EINVAL
    assert b'misaligned' in lib.lt_last_error()
