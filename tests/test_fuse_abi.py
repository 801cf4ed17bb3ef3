"""CPU-side checks of comet_pose_fuse (csrc/stream.hip): exported, declared, bound, and every bad
argument is reported through comet_last_error before anything is launched (no GPU needed)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

N_ARGS = 28


@pytest.fixture(scope="module")
def lib():
    from comet_amd import _lib
    return _lib.load()


class _Args:
    """Well-formed arguments over host memory (rejected calls never read the device pointers)."""

    def __init__(self, n=2, T=3, rows=8, slots=None, fresh=None, first=None, ratio=0.5, ratio_dev=False):
        self.buf = ctypes.create_string_buffer(1 << 14)
        base = ctypes.addressof(self.buf) + (-ctypes.addressof(self.buf)) % 256
        p = [base + 512 * k for k in range(20)]
        m, h = max(n, 1) * max(T, 1), max(n, 1)
        self.slots = (ctypes.c_int32 * m)(*(slots if slots is not None else range(m)))
        self.fresh = (ctypes.c_int32 * h)(*(fresh if fresh is not None else [1] * h))
        self.first = (ctypes.c_int32 * h)(*(first if first is not None else [1] * h))
        # enc, slots, slots_host, fresh, fresh_host, first, first_host, anchors, weights, ratio, ratio_dev,
        # fx, fy, cx, cy, acc, rows, n, T, R, uvz, T, count, rot_spread, trans_spread, hyp_R, hyp_T, stream
        self.a = [p[0], p[1], ctypes.addressof(self.slots), p[2], ctypes.addressof(self.fresh), p[3],
                  ctypes.addressof(self.first), p[4], None, ratio, p[5] if ratio_dev else None,
                  268.4, 268.4, 320.0, 240.0, p[6], rows, n, T, p[7], p[8], p[9], p[10], p[11], p[12], p[13], p[14], None]
        assert len(self.a) == N_ARGS


def _call(lib, args):
    return lib.comet_pose_fuse(*args.a)


def test_pose_fuse_is_exported_declared_and_bound(lib):
    from comet_amd import _lib
    src = open(os.path.join(ROOT, "include", "comet_hip.h")).read()
    m = re.search(r"^\s*int\s+comet_pose_fuse\((.*?)\);", src, re.M | re.S)
    assert m, "comet_pose_fuse is not declared in include/comet_hip.h"
    params = [a.strip() for a in m.group(1).split(",")]
    res, argtypes = _lib.SIGNATURES["comet_pose_fuse"]
    assert res is ctypes.c_int and len(params) == len(argtypes) == N_ARGS
    for prm, ty in zip(params, argtypes):
        if "*" in prm:
            assert ty is ctypes.c_void_p, prm
        elif prm.startswith("double"):
            assert ty is ctypes.c_double, prm
        else:
            assert prm.startswith("int ") and ty is ctypes.c_int, prm
    assert hasattr(lib, "comet_pose_fuse")
    assert re.search(r"#define\s+COMET_FUSE_ROW\s+20\b", src) and _lib.FUSE_ROW == 20


# the pointers that must not be null: everything but weights (8), ratio_dev (10) and the stream (27)
@pytest.mark.parametrize("index", [0, 1, 2, 3, 4, 5, 6, 7, 15, 19, 20, 21, 22, 23, 24, 25, 26])
def test_pose_fuse_rejects_null_pointers(lib, index):
    args = _Args()
    args.a[index] = None
    assert _call(lib, args) == -1
    assert b"comet_pose_fuse: null pointer" in lib.comet_last_error()


@pytest.mark.parametrize("n", [0, -1])
def test_pose_fuse_rejects_nonpositive_n(lib, n):
    assert _call(lib, _Args(n=n)) == -1
    assert b"comet_pose_fuse: n must be positive" in lib.comet_last_error()


@pytest.mark.parametrize("T", [1, 0, -3])
def test_pose_fuse_rejects_windows_below_2(lib, T):
    assert _call(lib, _Args(T=T)) == -1
    assert b"comet_pose_fuse: T must be at least 2" in lib.comet_last_error()


@pytest.mark.parametrize("rows", [0, -8])
def test_pose_fuse_rejects_nonpositive_rows(lib, rows):
    assert _call(lib, _Args(rows=rows)) == -1
    assert b"comet_pose_fuse: rows must be positive" in lib.comet_last_error()


@pytest.mark.parametrize("fresh", [[1, 0], [4, 1], [-1, 2], [2, 1 << 30]])
def test_pose_fuse_rejects_fresh_from_outside_1_to_T(lib, fresh):
    assert _call(lib, _Args(fresh=fresh, first=[0, 0])) == -1
    assert b"comet_pose_fuse: fresh_from outside [1, T]" in lib.comet_last_error()


@pytest.mark.parametrize("fresh,first", [([1, 1], [1, 2]), ([1, 1], [-1, 0]), ([2, 1], [1, 1])])
def test_pose_fuse_rejects_bad_first_flags(lib, fresh, first):
    """first is 0 or 1, and a first hop overwrites every position (fresh_from 1)."""
    assert _call(lib, _Args(fresh=fresh, first=first)) == -1
    assert b"comet_pose_fuse: first must be 0 or 1" in lib.comet_last_error()


@pytest.mark.parametrize("slots", [[0, 1, 2, 3, 4, 8], [0, -1, 2, 3, 4, 5], [1 << 30, 1, 2, 3, 4, 5]])
def test_pose_fuse_range_checks_slots_on_the_host(lib, slots):
    assert _call(lib, _Args(slots=slots)) == -1
    assert b"comet_pose_fuse: slot index outside the ring" in lib.comet_last_error()


@pytest.mark.parametrize("slots", [[0, 1, 2, 3, 4, 0], [5, 5, 2, 3, 4, 1], [0, 1, 2, 2, 4, 5]])
def test_pose_fuse_rejects_two_positions_for_one_row(lib, slots):
    """Two hops sharing a row (or one hop naming a row twice) would race."""
    assert _call(lib, _Args(slots=slots)) == -1
    assert b"comet_pose_fuse: duplicate slot index" in lib.comet_last_error()


@pytest.mark.parametrize("ratio", [0.0, -0.5, float("nan"), float("inf"), -float("inf")])
def test_pose_fuse_rejects_a_bad_host_ratio(lib, ratio):
    assert _call(lib, _Args(ratio=ratio)) == -1
    assert b"comet_pose_fuse: ratio must be finite and positive" in lib.comet_last_error()


def test_pose_fuse_checks_in_the_documented_order(lib):
    """Everything wrong at once: the null pointer is reported; with pointers, n; then T."""
    args = _Args(n=0, T=1, rows=0, ratio=-1.0)
    args.a[0] = None
    assert _call(lib, args) == -1 and b"null pointer" in lib.comet_last_error()
    assert _call(lib, _Args(n=0, T=1, rows=0, ratio=-1.0)) == -1 and b"n must be positive" in lib.comet_last_error()
    assert _call(lib, _Args(n=1, T=1, rows=0, ratio=-1.0)) == -1 and b"T must be at least 2" in lib.comet_last_error()
