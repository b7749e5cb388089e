"""_lib.call / _lib.size without a GPU: argument translation, device and status rules against a stub in place of the loaded library, and the
host-only entry points of the real one."""
import ctypes
import os

import pytest
import torch

from hybridneuralrendering_amd import _lib
from hybridneuralrendering_amd._lib import HnrError


class Stub:
    """Stands where the loaded library stands: every hnr_* attribute records its arguments and returns `status`."""

    def __init__(self, status=0, error=b"the stub's error text"):
        self.status, self.error, self.calls = status, error, []

    def hnr_last_error(self):
        return self.error

    def __getattr__(self, name):
        if not name.startswith("hnr_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            return self.status
        return fn


@pytest.fixture
def stub(monkeypatch):
    s = Stub()
    monkeypatch.setattr(_lib, "_lib", s)
    return s


@pytest.fixture
def real():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def test_cpu_tensor_is_refused_with_function_and_position(stub):
    with pytest.raises(HnrError, match=r"hnr_points_bounds.*argument 2"):
        _lib.call("hnr_points_bounds", None, 5, torch.zeros(6), None)
    with pytest.raises(HnrError, match=r"hnr_linear_f32.*argument 0"):
        _lib.call("hnr_linear_f32", _lib.Strided(torch.zeros(4, 4)), 4)
    assert stub.calls == []


def test_status_is_checked(stub):
    stub.status = -3
    with pytest.raises(HnrError, match=r"hnr_grid_free.*-3.*the stub's error text"):
        _lib.call("hnr_grid_free", 1234)
    assert stub.calls == [("hnr_grid_free", (1234,))]


def test_ok_status_is_returned(stub):
    stub.status = 1
    assert _lib.call("hnr_grid_free", 1234, ok=(1,)) == 1
    with pytest.raises(HnrError):
        _lib.call("hnr_grid_free", 1234, ok=(2,))
    stub.status = 0
    assert _lib.call("hnr_grid_free", 1234, ok=(1,)) == 0


def test_unknown_function_is_an_hnr_error(stub):
    with pytest.raises(HnrError, match="hnr_no_such_function"):
        _lib.call("hnr_no_such_function", 1)
    with pytest.raises(HnrError, match="hnr_no_such_size"):
        _lib.size("hnr_no_such_size", 1)
    assert stub.calls == []


def test_stream_needs_a_device(stub):
    with pytest.raises(HnrError, match="hnr_points_bounds.*device"):
        _lib.call("hnr_points_bounds", None, 0, None, _lib.STREAM)
    assert stub.calls == []


def test_structure_goes_by_reference_and_none_stays_none(stub):
    st = _lib.GridStats()
    assert _lib.call("hnr_grid_get_stats", None, st, 7, 0.5) == 0
    (name, args), = stub.calls
    assert name == "hnr_grid_get_stats" and args[0] is None and args[2:] == (7, 0.5)
    assert type(args[1]) is type(ctypes.byref(st)) and args[1]._obj is st


def test_packed_dims_of_the_real_library(real):
    a, b, c, d = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert _lib.call("hnr_linear_packed_dims", 45, 284, ctypes.byref(a), ctypes.byref(b)) == 0
    assert real.hnr_linear_packed_dims(45, 284, ctypes.byref(c), ctypes.byref(d)) == 0
    assert (a.value, b.value) == (c.value, d.value) and a.value >= 45 and b.value >= 284


def test_size_of_the_real_library(real):
    with pytest.raises(HnrError, match="hnr_raft_encoder_scratch_elems"):
        _lib.size("hnr_raft_encoder_scratch_elems", 3, 128, 128)               # N = 3: the library answers -1
    with pytest.raises(HnrError, match="my own words"):
        _lib.size("hnr_raft_encoder_scratch_elems", 3, 128, 128, what="my own words")
    n = _lib.size("hnr_raft_encoder_scratch_elems", 2, 128, 128)
    assert type(n) is int and n > 0 and n == real.hnr_raft_encoder_scratch_elems(2, 128, 128)


def test_size_refuses_an_int_outside_its_c_type(real, stub):
    for args in ((2, 2 ** 31, 128), (2, 128, -2 ** 31 - 1)):
        with pytest.raises(HnrError, match="hnr_raft_encoder_scratch_elems"):
            _lib.size("hnr_raft_encoder_scratch_elems", *args)
    with pytest.raises(HnrError):
        _lib.size("hnr_range_crop_scratch_bytes", 2 ** 63)                      # an int64_t parameter
    assert stub.calls == []
    stub.status = 48
    assert _lib.size("hnr_range_crop_scratch_bytes", 2 ** 31) == 48             # in range for int64_t
