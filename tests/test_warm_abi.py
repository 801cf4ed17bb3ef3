"""CPU-side checks of comet_track_warm (csrc/warm.hip): exported, declared, bound, and every bad
argument is reported through comet_last_error before anything is launched (no GPU needed)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

N_ARGS = 16
# prev, src, query, prev_valid, n, T, N, s, H, W, mode, div0, div1, coords, warm, stream
IDX = {"prev": 0, "src": 1, "query": 2, "prev_valid": 3, "n": 4, "T": 5, "N": 6, "s": 7, "H": 8, "W": 9, "mode": 10,
       "div0": 11, "div1": 12, "coords": 13, "warm": 14}


@pytest.fixture(scope="module")
def lib():
    from comet_amd import _lib
    return _lib.load()


class _Args:
    """Well-formed arguments over host memory (rejected calls never read the device pointers)."""

    def __init__(self, **kw):
        self.buf = ctypes.create_string_buffer(1 << 13)
        base = ctypes.addressof(self.buf) + (-ctypes.addressof(self.buf)) % 256
        p = [base + 512 * k for k in range(6)]
        v = dict(n=2, T=4, N=64, s=1, H=128, W=128, mode=0, div0=2.0, div1=4.0)
        v.update(kw)
        self.a = [p[0], p[1], p[2], p[3], v["n"], v["T"], v["N"], v["s"], v["H"], v["W"], v["mode"], v["div0"],
                  v["div1"], p[4], p[5], None]
        assert len(self.a) == N_ARGS


def _call(lib, args):
    return lib.comet_track_warm(*args.a)


def _rejected(lib, message, **kw):
    assert _call(lib, _Args(**kw)) == -1
    assert message in lib.comet_last_error(), lib.comet_last_error()


def test_track_warm_is_exported_declared_and_bound(lib):
    from comet_amd import _lib
    src = open(os.path.join(ROOT, "include", "comet_hip.h")).read()
    m = re.search(r"^\s*int\s+comet_track_warm\((.*?)\);", src, re.M | re.S)
    assert m, "comet_track_warm is not declared in include/comet_hip.h"
    params = [a.strip() for a in m.group(1).split(",")]
    res, argtypes = _lib.SIGNATURES["comet_track_warm"]
    assert res is ctypes.c_int and len(params) == len(argtypes) == N_ARGS
    for prm, ty in zip(params, argtypes):
        if "*" in prm:
            assert ty is ctypes.c_void_p, prm
        elif prm.startswith("float"):
            assert ty is ctypes.c_float, prm
        else:
            assert prm.startswith("int ") and ty is ctypes.c_int, prm
    assert hasattr(lib, "comet_track_warm")
    assert [p.split()[-1].lstrip("*") for p in params[:15]] == list(IDX)


# the pointers that must not be null: everything but the stream (15)
@pytest.mark.parametrize("index", [0, 1, 2, 3, 13, 14])
def test_track_warm_rejects_null_pointers(lib, index):
    args = _Args()
    args.a[index] = None
    assert _call(lib, args) == -1
    assert b"comet_track_warm: null pointer" in lib.comet_last_error()


@pytest.mark.parametrize("n", [0, -1])
def test_track_warm_rejects_nonpositive_n(lib, n):
    _rejected(lib, b"comet_track_warm: n must be positive", n=n)


@pytest.mark.parametrize("N", [0, -5, 4097, 1 << 30])
def test_track_warm_rejects_track_counts_outside_1_to_4096(lib, N):
    from comet_amd import _lib
    assert _lib.CARRY_MAX_TRACKS == 4096
    _rejected(lib, b"comet_track_warm: N outside [1, 4096]", N=N)


@pytest.mark.parametrize("T", [1, 0, -3])
def test_track_warm_rejects_windows_below_two_frames(lib, T):
    _rejected(lib, b"comet_track_warm: T must be at least 2", T=T, s=1)


@pytest.mark.parametrize("s,T", [(0, 4), (4, 4), (-1, 4), (7, 4), (2, 2)])
def test_track_warm_rejects_a_stride_outside_the_window(lib, s, T):
    _rejected(lib, b"comet_track_warm: s outside [1, T - 1]", s=s, T=T)


@pytest.mark.parametrize("H,W", [(0, 128), (128, 0), (-4, 128), (128, -1)])
def test_track_warm_rejects_empty_frames(lib, H, W):
    _rejected(lib, b"comet_track_warm: H and W must be positive", H=H, W=W)


@pytest.mark.parametrize("mode", [-1, 2, 7])
def test_track_warm_rejects_unknown_modes(lib, mode):
    _rejected(lib, b"comet_track_warm: mode must be 0 (hold) or 1 (constant velocity)", mode=mode)


@pytest.mark.parametrize("div0,div1", [(0.0, 4.0), (2.0, 0.0), (-2.0, 4.0), (2.0, -1.0), (float("nan"), 4.0),
                                       (2.0, float("nan")), (float("inf"), 4.0), (2.0, float("inf"))])
def test_track_warm_rejects_divisors_that_are_not_finite_and_positive(lib, div0, div1):
    _rejected(lib, b"comet_track_warm: div0 and div1 must be finite and positive", div0=div0, div1=div1)


@pytest.mark.parametrize("name", ["prev", "query", "coords"])
def test_track_warm_rejects_misaligned_points(lib, name):
    args = _Args()
    args.a[IDX[name]] += 4
    assert _call(lib, args) == -1
    assert b"comet_track_warm: prev, query and coords must be 8-B aligned" in lib.comet_last_error()


def test_track_warm_checks_in_the_documented_order(lib):
    """Everything wrong at once: the null pointer is reported; with pointers, n; then N, T, s, H / W,
    mode, the divisors."""
    bad = dict(n=0, N=0, T=1, s=0, H=0, mode=3, div0=0.0)
    args = _Args(**bad)
    args.a[0] = None
    assert _call(lib, args) == -1 and b"null pointer" in lib.comet_last_error()
    fixes = [("n must be positive", dict(n=1)), ("N outside", dict(N=8)), ("T must be at least 2", dict(T=3)),
             ("s outside", dict(s=2)), ("H and W", dict(H=16)), ("mode must be", dict(mode=1)),
             ("div0 and div1", dict(div0=1.0))]
    for message, fix in fixes:
        assert _call(lib, _Args(**bad)) == -1 and message.encode() in lib.comet_last_error(), message
        bad.update(fix)
    args = _Args(**bad)
    args.a[IDX["query"]] += 4
    assert _call(lib, args) == -1 and b"8-B aligned" in lib.comet_last_error()
