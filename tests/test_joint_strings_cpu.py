"""The C ABI of the joint string rows without a GPU: include/lt_joint_strings.h
declares the two entry points, the library exports them, the binding lists
them, and lt_lattice.h pulls the header in."""
import os
import re

from last_torch_amd import _native

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include')


def test_library_exports_what_lt_joint_strings_h_declares():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(INCLUDE, 'lt_joint_strings.h')).read(),
               flags=re.S)
  declared = sorted(set(re.findall(r'\b(lt_[a-z_]+)\s*\(', src)))
  assert declared == sorted(_native.EXPORTED_JOINT_STRINGS) and len(declared) == 2
  for name in declared:
    assert hasattr(_native.lib(), name) and name in _native._SIG
    assert name not in _native.EXPORTED


def test_lt_lattice_h_includes_the_header():
  assert '#include "lt_joint_strings.h"' in open(os.path.join(INCLUDE, 'lt_lattice.h')).read()
