"""CPU-side checks of comet_ring_scatter (csrc/stream.hip): exported, declared, bound, and every bad
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


def _args(n=1, slot_bytes=64, k=3, capacity=8, slots=None):
    """Well-formed arguments over host memory (rejected calls never read it)."""
    from comet_amd import _lib
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256
    R = (_lib.RingTensor * max(n, 1))()
    for r in R:
        r.src, r.dst, r.slot_bytes = p, p + 1024, slot_bytes
    host = (ctypes.c_int32 * max(k, 1))(*(slots if slots is not None else [i % capacity for i in range(max(k, 1))]))
    return buf, R, n, p + 2048, ctypes.addressof(host), host, k, capacity


def _call(lib, a, max_blocks=0):
    buf, R, n, dev_slots, host_ptr, host, k, cap = a
    return lib.comet_ring_scatter(R, n, dev_slots, host_ptr, k, cap, max_blocks, None)


def test_ring_scatter_is_exported_declared_and_bound(lib):
    from comet_amd import _lib
    src = open(os.path.join(ROOT, "include", "comet_hip.h")).read()
    assert re.search(r"^\s*int\s+comet_ring_scatter\(", src, re.M)
    assert hasattr(lib, "comet_ring_scatter")
    assert "comet_ring_scatter" in _lib.SIGNATURES
    assert _lib.SIGNATURES["comet_ring_scatter"] == _lib.SIGNATURES["comet_ring_gather"]


def test_ring_scatter_rejects_null_pointers(lib):
    buf, R, n, dev_slots, host_ptr, host, k, cap = _args()
    assert lib.comet_ring_scatter(None, n, dev_slots, host_ptr, k, cap, 0, None) == -1
    assert b"comet_ring_scatter: null pointer" in lib.comet_last_error()
    assert lib.comet_ring_scatter(R, n, None, host_ptr, k, cap, 0, None) == -1
    assert b"null pointer" in lib.comet_last_error()
    assert lib.comet_ring_scatter(R, n, dev_slots, None, k, cap, 0, None) == -1
    assert b"null pointer" in lib.comet_last_error()
    for field in ("src", "dst"):
        a = _args(n=2)
        setattr(a[1][1], field, None)
        assert _call(lib, a) == -1
        assert b"comet_ring_scatter: null tensor" in lib.comet_last_error()


@pytest.mark.parametrize("n", [0, 5, 9])
def test_ring_scatter_rejects_tensor_counts_outside_1_to_4(lib, n):
    a = _args(n=max(n, 1))
    a = a[:2] + (n,) + a[3:]
    assert _call(lib, a) == -1
    assert b"comet_ring_scatter: 1 to 4 tensors" in lib.comet_last_error()


@pytest.mark.parametrize("k", [0, -1])
def test_ring_scatter_rejects_nonpositive_k(lib, k):
    assert _call(lib, _args(k=k)) == -1
    assert b"comet_ring_scatter: k must be positive" in lib.comet_last_error()


def test_ring_scatter_rejects_capacity_below_k(lib):
    assert _call(lib, _args(k=6, capacity=5)) == -1
    assert b"comet_ring_scatter: capacity below k" in lib.comet_last_error()


def test_ring_scatter_rejects_negative_max_blocks(lib):
    assert _call(lib, _args(), max_blocks=-1) == -1
    assert b"comet_ring_scatter: negative max_blocks" in lib.comet_last_error()


@pytest.mark.parametrize("slot_bytes", [0, 8, 24, 4100, -16])
def test_ring_scatter_rejects_slot_bytes_not_multiple_of_16(lib, slot_bytes):
    assert _call(lib, _args(slot_bytes=slot_bytes)) == -1
    assert b"comet_ring_scatter: slot_bytes must be a positive multiple of 16" in lib.comet_last_error()


@pytest.mark.parametrize("field", ["src", "dst"])
def test_ring_scatter_rejects_misaligned_pointers(lib, field):
    a = _args()
    setattr(a[1][0], field, getattr(a[1][0], field) + 8)
    assert _call(lib, a) == -1
    assert b"comet_ring_scatter: pointers must be 16-B aligned" in lib.comet_last_error()


def test_ring_scatter_rejects_a_slot_too_large_for_32_bit_vector_counts(lib):
    assert _call(lib, _args(slot_bytes=16 << 31)) == -1
    assert b"comet_ring_scatter: slot too large" in lib.comet_last_error()


@pytest.mark.parametrize("slots", [[5, 0, 8], [5, -1, 7], [1 << 30, 0, 1]])
def test_ring_scatter_range_checks_slots_on_the_host(lib, slots):
    assert _call(lib, _args(slots=slots)) == -1
    assert b"comet_ring_scatter: slot index outside the ring" in lib.comet_last_error()


@pytest.mark.parametrize("slots", [[5, 0, 5], [7, 7, 0], [2, 2, 2]])
def test_ring_scatter_rejects_two_sources_for_one_slot(lib, slots):
    """Two rows written to one slot would race."""
    assert _call(lib, _args(slots=slots)) == -1
    assert b"comet_ring_scatter: duplicate slot index" in lib.comet_last_error()
