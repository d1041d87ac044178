"""Device-resident input and output without a device (docs/DEVICE_IO.md): device_matrix -- the pure-Python step that turns a device array's
__cuda_array_interface__ into the (ptr, ld, layout) the C entries take -- on hand-made interfaces, every accepted stride form and every refusal; and the five new
entries in the header and in the built library."""
import os
import re

import numpy as np
import pytest

import nmfgpu_amd as na

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x7F0000001000
ENTRIES = ("nmfamd_engine_upload_dense_device", "nmfamd_engine_upload_dense_weighted_device", "nmfamd_engine_set_factors_device",
           "nmfamd_engine_get_factors_device", "nmfamd_device_pointer_info")


class Fake:
    """An object that carries a __cuda_array_interface__ and nothing else (strides in bytes, as the protocol has them)."""

    def __init__(self, shape, typestr="<f4", strides=None, ptr=PTR, read_only=False):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, read_only), "strides": strides, "version": 2}


def test_contiguous_forms_are_row_major():
    assert na.device_matrix(Fake((130, 257)), (130, 257), np.float32) == (PTR, 257, na.ROW_MAJOR)
    assert na.device_matrix(Fake((130, 257), strides=(257 * 4, 4)), (130, 257), np.float32) == (PTR, 257, na.ROW_MAJOR)
    assert na.device_matrix(Fake((130, 257), "<f8", strides=(257 * 8, 8)), (130, 257), np.float64) == (PTR, 257, na.ROW_MAJOR)


def test_padded_and_transposed_forms():
    # a slice of a wider row-major array: ld = 262
    assert na.device_matrix(Fake((130, 257), strides=(262 * 4, 4)), (130, 257), np.float32) == (PTR, 262, na.ROW_MAJOR)
    # the .T view of a contiguous (257, 130) array: column-major with ld = 130
    assert na.device_matrix(Fake((130, 257), strides=(4, 130 * 4)), (130, 257), np.float32) == (PTR, 130, na.COLUMN_MAJOR)
    # ... of a taller one: ld = 133, float64
    assert na.device_matrix(Fake((130, 257), "<f8", strides=(8, 133 * 8)), (130, 257), np.float64) == (PTR, 133, na.COLUMN_MAJOR)
    # a pointer one element into its buffer stays what it is
    assert na.device_matrix(Fake((130, 257), strides=(257 * 4, 4), ptr=PTR + 4), (130, 257), np.float32)[0] == PTR + 4
    # numpy's own strides agree for a .T view
    a = np.zeros((257, 130), np.float32).T
    assert na.device_matrix(Fake(a.shape, strides=a.strides), (130, 257), np.float32)[1:] == (130, na.COLUMN_MAJOR)


def test_single_row_and_single_column():
    assert na.device_matrix(Fake((1, 7), strides=(28, 4)), (1, 7), np.float32) == (PTR, 7, na.ROW_MAJOR)
    assert na.device_matrix(Fake((7, 1), strides=(4, 28)), (7, 1), np.float32) == (PTR, 7, na.COLUMN_MAJOR)
    assert na.device_matrix(Fake((7, 1), strides=(4, 4)), (7, 1), np.float32) == (PTR, 1, na.ROW_MAJOR)
    assert na.device_matrix(Fake((1, 7), strides=(4, 4)), (1, 7), np.float32) == (PTR, 1, na.COLUMN_MAJOR)


def test_writable():
    assert na.device_matrix(Fake((4, 5)), (4, 5), np.float32, writable=True) == (PTR, 5, na.ROW_MAJOR)
    assert na.device_matrix(Fake((4, 5), read_only=True), (4, 5), np.float32) == (PTR, 5, na.ROW_MAJOR)
    with pytest.raises(TypeError):
        na.device_matrix(Fake((4, 5), read_only=True), (4, 5), np.float32, writable=True)


@pytest.mark.parametrize("obj, shape, dtype, error", [
    (np.zeros((4, 5), np.float32), (4, 5), np.float32, TypeError),                # no interface
    (object(), (4, 5), np.float32, TypeError),
    (Fake((4, 5), "<f8"), (4, 5), np.float32, TypeError),                         # another dtype
    (Fake((4, 5), "<f4"), (4, 5), np.float64, TypeError),
    (Fake((4, 5), "<i4"), (4, 5), np.float32, TypeError),
    (Fake((5, 4)), (4, 5), np.float32, ValueError),                               # another shape
    (Fake((20,)), (4, 5), np.float32, ValueError),
    (Fake((4, 5), strides=(40, 8)), (4, 5), np.float32, ValueError),              # both strides non-unit (every second column)
    (Fake((4, 5), strides=(0, 4)), (4, 5), np.float32, ValueError),               # a zero stride (a broadcast row)
    (Fake((4, 5), strides=(20, -4)), (4, 5), np.float32, ValueError),             # a negative stride
    (Fake((4, 5), strides=(22, 4)), (4, 5), np.float32, ValueError),              # not a multiple of the item size
    (Fake((4, 5), strides=(16, 4)), (4, 5), np.float32, ValueError),              # rows that overlap: ld 4 < 5 columns
    (Fake((4, 5), strides=(4, 12)), (4, 5), np.float32, ValueError),              # columns that overlap: ld 3 < 4 rows
])
def test_refusals(obj, shape, dtype, error):
    with pytest.raises(error):
        na.device_matrix(obj, shape, dtype)


def test_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "nmfgpu_amd.h")).read()
    lib = na.library()
    for name in ENTRIES:
        assert re.search(r"NMFAMD_API\s+int\s+" + name + r"\s*\(", header), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
    assert re.search(r"NMFAMD_COLUMN_MAJOR\s*=\s*0\s*,\s*NMFAMD_ROW_MAJOR\s*=\s*1", header)
    assert (na.COLUMN_MAJOR, na.ROW_MAJOR) == (0, 1)
    for name in ("upload_device", "set_factors_device", "get_factors_device"):
        assert callable(getattr(na.Engine, name))
    # the ctypes mirror and the document name the same entries
    mirror = open(os.path.join(ROOT, "nmfgpu_amd", "engine.py")).read()
    doc = open(os.path.join(ROOT, "docs", "DEVICE_IO.md")).read()
    for name in ENTRIES:
        assert name in mirror and name in doc, name
