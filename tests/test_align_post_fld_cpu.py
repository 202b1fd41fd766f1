"""lt_table_align_posteriors_fld's host validation (no GPU: nothing below
launches or dereferences a device pointer): its range, the workspace rule, the
NULL rules, and that the library exports what include/lt_posterior_fld.h
declares."""
import ctypes
import os
import re

from last_torch_amd import _native
from abi_graph import dummy_graph

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include')
OK, EINVAL, EUNSUPPORTED = 0, -1, -2  # LT_OK, LT_EINVAL, LT_EUNSUPPORTED (lt_lattice.h)


def test_library_exports_what_lt_posterior_fld_h_declares():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(INCLUDE, 'lt_posterior_fld.h')).read(),
               flags=re.S)
  declared = sorted(set(re.findall(r'\b(lt_[a-z_]+)\s*\(', src)))
  assert declared == sorted(_native.EXPORTED_POSTERIOR_FLD) and len(declared) == 2
  for name in declared:
    assert hasattr(_native.lib(), name) and name in _native._SIG
    assert name not in _native.EXPORTED
  assert '#include "lt_posterior_fld.h"' in open(os.path.join(INCLUDE, 'lt_posterior.h')).read()


def test_fld_align_posteriors_host_validation_error_codes():
  lib = _native.lib()
  null = ctypes.c_void_p(0)
  buf = (ctypes.c_int64 * 64)()  # stands in for the device pointers
  p = ctypes.c_void_p(ctypes.addressof(buf))
  TP = _native.TableProblem

  def call(g, pb, lp=p, ws=p, nbytes=1 << 40):
    return lib.lt_table_align_posteriors_fld(ctypes.byref(g), ctypes.byref(pb), p, p, p, p, p, lp,
                                             ws, nbytes, null)

  def query(g, pb, nbytes):
    return lib.lt_table_align_posteriors_fld_workspace_bytes(ctypes.byref(g), ctypes.byref(pb),
                                                             ctypes.byref(nbytes))

  nbytes = ctypes.c_size_t(7)
  for K, U in ((0, 9), (16, 9), (2, 256)):  # K = 0 is lt_table_align_posteriors' own
    pb = TP(batch=2, max_frames=4, max_labels=U, weight_dtype=0)
    assert query(dummy_graph(p, K=K), pb, nbytes) == EUNSUPPORTED
    assert call(dummy_graph(p, K=K), pb) == EUNSUPPORTED
  assert nbytes.value == 7  # a refused query writes nothing
  for K in (1, 15):
    # 76 rows of 8 * 256 bytes fit LDS beside the prologue's arrays; from the 77th the history
    # is the workspace's: batch * max_frames * 256 * 8 bytes, whatever K is
    for T, want in ((76, 0), (77, 3 * 77 * 256 * 8)):
      pb = TP(batch=3, max_frames=T, max_labels=255, weight_dtype=1)
      assert query(dummy_graph(p, K=K), pb, nbytes) == OK and nbytes.value == want
    assert call(dummy_graph(p, K=K), pb, lp=null) == EINVAL
    assert b'null pointer' in lib.lt_last_error()
    assert call(dummy_graph(p, K=K), pb, nbytes=nbytes.value - 1) == EINVAL
    assert b'workspace' in lib.lt_last_error()
