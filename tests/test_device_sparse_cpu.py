"""Device-resident sparse input without a device (docs/DEVICE_IO.md): device_vector -- the pure-Python step that turns a 1-D device array's
__cuda_array_interface__ (or a raw pair) into the (ptr, count) the sparse device entry takes -- on hand-made interfaces, every accepted form and every refusal;
and the two new entries in the header and in the built library."""
import os
import re

import numpy as np
import pytest

import nmfgpu_amd as na

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x7F0000002000
ENTRIES = ("nmfamd_engine_upload_sparse_device", "nmfamd_engine_upload_dense_device_stored")


class Fake:
    """An object that carries a __cuda_array_interface__ and nothing else (strides in bytes, as the protocol has them)."""

    def __init__(self, shape, typestr="<f4", strides=None, ptr=PTR):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "strides": strides, "version": 2}


def test_accepted_forms():
    assert na.device_vector(Fake((100,)), np.float32) == (PTR, 100)
    assert na.device_vector(Fake((100,), strides=(4,)), np.float32) == (PTR, 100)
    assert na.device_vector(Fake((100,), "<f8", strides=(8,)), np.float64, 100) == (PTR, 100)
    assert na.device_vector(Fake((518,), "<i4"), np.int32, 518) == (PTR, 518)
    assert na.device_vector(Fake((7,), "<i4", ptr=PTR + 4), np.int32) == (PTR + 4, 7)      # a pointer one element into its buffer stays what it is
    assert na.device_vector(Fake((0,), "<i4", ptr=0), np.int32, 0) == (0, 0)               # an empty array (a null pointer travels as 0)
    # a raw pair goes through as it is: the library checks that one
    assert na.device_vector((PTR, 12), np.float32) == (PTR, 12)
    assert na.device_vector((PTR, 12), np.int32, 12) == (PTR, 12)
    assert na.device_vector((None, 0), np.int32) == (0, 0)
    # numpy's own strides agree for a contiguous array
    a = np.zeros(9, np.int32)
    assert na.device_vector(Fake(a.shape, "<i4", strides=a.strides), np.int32) == (PTR, 9)


@pytest.mark.parametrize("obj, dtype, count, error", [
    (np.zeros(5, np.float32), np.float32, None, TypeError),                # no interface
    (object(), np.float32, None, TypeError),
    (Fake((5,), "<f8"), np.float32, None, TypeError),                      # another dtype
    (Fake((5,), "<f4"), np.float64, None, TypeError),
    (Fake((5,), "<f4"), np.int32, None, TypeError),
    (Fake((5,), "<i8"), np.int32, None, TypeError),                        # torch's CSR default
    (Fake((5, 1)), np.float32, None, ValueError),                          # another rank
    (Fake((), "<f4"), np.float32, None, ValueError),
    (Fake((5,), strides=(8,)), np.float32, None, ValueError),              # every second element
    (Fake((5,), strides=(0,)), np.float32, None, ValueError),              # a broadcast element
    (Fake((5,), strides=(-4,)), np.float32, None, ValueError),             # reversed
    (Fake((5,)), np.float32, 6, ValueError),                               # a count that differs
    ((PTR, 5), np.float32, 6, ValueError),
])
def test_refusals(obj, dtype, count, error):
    with pytest.raises(error):
        na.device_vector(obj, dtype, count)


def test_int64_indices_are_told_to_convert():
    with pytest.raises(TypeError, match="int32"):
        na.device_vector(Fake((5,), "<i8"), np.int32)
    with pytest.raises(TypeError) as e:
        na.device_vector(Fake((5,), "<f8"), np.float32)
    assert "convert" not in str(e.value)


def test_nothing_imports_torch():
    mirror = open(os.path.join(ROOT, "nmfgpu_amd", "engine.py")).read()
    assert not re.search(r"^\s*(import|from)\s+torch\b", mirror, re.M)


def test_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "nmfgpu_amd.h")).read()
    lib = na.library()
    for name in ENTRIES:
        assert re.search(r"NMFAMD_API\s+int\s+" + name + r"\s*\(", header), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
    for name in ("upload_sparse_device", "upload_device_stored"):
        assert callable(getattr(na.Engine, name))
    # the ctypes mirror and the document name the same entries
    mirror = open(os.path.join(ROOT, "nmfgpu_amd", "engine.py")).read()
    doc = open(os.path.join(ROOT, "docs", "DEVICE_IO.md")).read()
    for name in ENTRIES:
        assert name in mirror and name in doc, name
