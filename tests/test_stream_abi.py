"""CPU-side checks of comet_ring_gather (csrc/stream.hip): exported, declared, bound, and every bad
argument is reported through comet_last_error before anything is launched (no GPU needed)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from comet_amd import _lib
    return _lib.load()


def _args(n=1, slot_bytes=64, T=4, capacity=5, slots=None):
    """Well-formed arguments over host memory (rejected calls never read it)."""
    from comet_amd import _lib
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256
    R = (_lib.RingTensor * max(n, 1))()
    for r in R:
        r.src, r.dst, r.slot_bytes = p, p + 1024, slot_bytes
    host = (ctypes.c_int32 * max(T, 1))(*(slots if slots is not None else [i % capacity for i in range(max(T, 1))]))
    return buf, R, n, p + 2048, ctypes.addressof(host), host, T, capacity


def _call(lib, a, max_blocks=0):
    buf, R, n, dev_slots, host_ptr, host, T, cap = a
    return lib.comet_ring_gather(R, n, dev_slots, host_ptr, T, cap, max_blocks, None)


def test_ring_gather_is_exported_declared_and_bound(lib):
    from comet_amd import _lib
    src = open(os.path.join(ROOT, "include", "comet_hip.h")).read()
    assert re.search(r"^\s*int\s+comet_ring_gather\(", src, re.M)
    assert "COMET_RING_MAX_TENSORS 4" in src
    assert hasattr(lib, "comet_ring_gather")
    assert "comet_ring_gather" in _lib.SIGNATURES
    assert _lib.RING_MAX_TENSORS == 4
    assert ctypes.sizeof(_lib.RingTensor) == 24


def test_ring_gather_rejects_null_pointers(lib):
    a = _args()
    buf, R, n, dev_slots, host_ptr, host, T, cap = a
    assert lib.comet_ring_gather(None, n, dev_slots, host_ptr, T, cap, 0, None) == -1
    assert b"null pointer" in lib.comet_last_error()
    assert lib.comet_ring_gather(R, n, None, host_ptr, T, cap, 0, None) == -1
    assert b"null pointer" in lib.comet_last_error()
    assert lib.comet_ring_gather(R, n, dev_slots, None, T, cap, 0, None) == -1
    assert b"null pointer" in lib.comet_last_error()
    for field in ("src", "dst"):
        a = _args(n=2)
        setattr(a[1][1], field, None)
        assert _call(lib, a) == -1
        assert b"null tensor" in lib.comet_last_error()


@pytest.mark.parametrize("slot_bytes", [0, 8, 24, 4100, -16])
def test_ring_gather_rejects_slot_bytes_not_multiple_of_16(lib, slot_bytes):
    assert _call(lib, _args(slot_bytes=slot_bytes)) == -1
    assert b"multiple of 16" in lib.comet_last_error()


@pytest.mark.parametrize("T", [0, -1])
def test_ring_gather_rejects_nonpositive_T(lib, T):
    assert _call(lib, _args(T=T)) == -1
    assert b"T must be positive" in lib.comet_last_error()


@pytest.mark.parametrize("n", [0, 5, 9])
def test_ring_gather_rejects_tensor_counts_outside_1_to_4(lib, n):
    a = _args(n=max(n, 1))
    a = a[:2] + (n,) + a[3:]
    assert _call(lib, a) == -1
    assert b"1 to 4 tensors" in lib.comet_last_error()


def test_ring_gather_range_checks_slots_on_the_host(lib):
    for slots in ([0, 1, 2, 5], [0, -1, 2, 3]):
        assert _call(lib, _args(slots=slots)) == -1
        assert b"outside the ring" in lib.comet_last_error()
    assert _call(lib, _args(T=6, capacity=5)) == -1
    assert b"capacity below T" in lib.comet_last_error()


def test_ring_gather_rejects_misaligned_pointers(lib):
    a = _args()
    a[1][0].src += 8
    assert _call(lib, a) == -1
    assert b"16-B aligned" in lib.comet_last_error()
