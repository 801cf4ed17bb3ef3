"""CPU-side checks of comet_landmark_update (csrc/landmark.hip): exported, declared, bound, and every
bad argument is reported through comet_last_error before anything is launched (no GPU needed)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

N_ARGS = 25
NAMES = ["tracks", "weights", "R", "T", "ids", "src", "stream_idx", "stream_idx_host", "intr", "intr_host", "acc",
         "acc_id", "rows", "n", "Tw", "N", "s", "inverse_rotation", "min_obs", "min_pivot", "X", "n_obs", "err_px",
         "state"]
IDX = {name: i for i, name in enumerate(NAMES)}
POINTERS = [i for i, name in enumerate(NAMES) if name not in ("rows", "n", "Tw", "N", "s", "inverse_rotation",
                                                             "min_obs", "min_pivot")]


@pytest.fixture(scope="module")
def lib():
    from comet_amd import _lib
    return _lib.load()


class _Args:
    """Well-formed arguments over host memory (rejected calls never read the device pointers)."""

    def __init__(self, streams=None, intr=None, **kw):
        self.buf = ctypes.create_string_buffer(1 << 14)
        base = ctypes.addressof(self.buf) + (-ctypes.addressof(self.buf)) % 256
        p = {name: base + 512 * k for k, name in enumerate(NAMES[i] for i in POINTERS)}
        v = dict(rows=4 * 64, n=2, Tw=4, N=64, s=1, inverse_rotation=0, min_obs=3, min_pivot=1e-8)
        v.update(kw)
        n = max(v["n"], 1)
        streams = list(range(n)) if streams is None else streams
        intr = [(100.0, 110.0, 64.0, 64.0)] * n if intr is None else intr
        self.streams = (ctypes.c_int32 * len(streams))(*streams)
        flat = [x for row in intr for x in row]
        self.intr = (ctypes.c_double * len(flat))(*flat)
        p["stream_idx_host"], p["intr_host"] = ctypes.addressof(self.streams), ctypes.addressof(self.intr)
        self.a = [p[name] if name in p else v[name] for name in NAMES] + [None]
        assert len(self.a) == N_ARGS


def _call(lib, args):
    return lib.comet_landmark_update(*args.a)


def _rejected(lib, message, **kw):
    assert _call(lib, _Args(**kw)) == -1
    assert message in lib.comet_last_error(), lib.comet_last_error()


def test_landmark_update_is_exported_declared_and_bound(lib):
    from comet_amd import _lib
    src = open(os.path.join(ROOT, "include", "comet_hip.h")).read()
    m = re.search(r"^\s*int\s+comet_landmark_update\((.*?)\);", src, re.M | re.S)
    assert m, "comet_landmark_update is not declared in include/comet_hip.h"
    params = [a.strip() for a in m.group(1).split(",")]
    assert "comet_landmark_update" in _lib.SIGNATURES, "comet_landmark_update is not bound in comet_amd._lib"
    res, argtypes = _lib.SIGNATURES["comet_landmark_update"]
    assert res is ctypes.c_int and len(params) == len(argtypes) == N_ARGS
    for prm, ty in zip(params, argtypes):
        if "*" in prm:
            assert ty is ctypes.c_void_p, prm
        elif prm.startswith("double"):
            assert ty is ctypes.c_double, prm
        else:
            assert prm.startswith("int ") and ty is ctypes.c_int, prm
    assert hasattr(lib, "comet_landmark_update")
    assert [p.split()[-1].lstrip("*") for p in params[:24]] == NAMES
    assert re.search(r"#define\s+COMET_LM_ROW\s+12\b", src) and _lib.LM_ROW == 12


# the pointers that must not be null: everything but weights (1) and the stream (24)
@pytest.mark.parametrize("index", [i for i in POINTERS if i != 1])
def test_landmark_update_rejects_null_pointers(lib, index):
    args = _Args()
    args.a[index] = None
    assert _call(lib, args) == -1
    assert b"comet_landmark_update: null pointer" in lib.comet_last_error()


def test_landmark_update_null_weights_pass_the_pointer_check(lib):
    """weights may be null: with null weights and a bad n, the report is about n."""
    args = _Args(n=0)
    args.a[IDX["weights"]] = None
    assert _call(lib, args) == -1
    assert b"comet_landmark_update: n must be positive" in lib.comet_last_error()


@pytest.mark.parametrize("n", [0, -1])
def test_landmark_update_rejects_nonpositive_n(lib, n):
    _rejected(lib, b"comet_landmark_update: n must be positive", n=n)


@pytest.mark.parametrize("N", [0, -5, 4097, 1 << 30])
def test_landmark_update_rejects_track_counts_outside_1_to_4096(lib, N):
    _rejected(lib, b"comet_landmark_update: N outside [1, 4096]", N=N)


@pytest.mark.parametrize("T", [1, 0, -3])
def test_landmark_update_rejects_windows_below_two_frames(lib, T):
    _rejected(lib, b"comet_landmark_update: T must be at least 2", Tw=T, s=1)


@pytest.mark.parametrize("s,T", [(0, 4), (4, 4), (-1, 4), (7, 4), (2, 2)])
def test_landmark_update_rejects_a_stride_outside_the_window(lib, s, T):
    _rejected(lib, b"comet_landmark_update: s outside [1, T - 1]", s=s, Tw=T)


@pytest.mark.parametrize("rows,n,N", [(127, 2, 64), (0, 1, 1), (-64, 1, 64), (64, 2, 64)])
def test_landmark_update_rejects_a_state_smaller_than_the_hops(lib, rows, n, N):
    _rejected(lib, b"comet_landmark_update: rows below n * N", rows=rows, n=n, N=N)


@pytest.mark.parametrize("streams", [[0, 4], [-1, 0], [4, 5], [1 << 20, 0]])
def test_landmark_update_rejects_stream_indices_outside_the_state(lib, streams):
    _rejected(lib, b"comet_landmark_update: stream index outside the state", streams=streams)  # rows / N = 4


def test_landmark_update_rejects_rows_that_end_in_a_partial_stream(lib):
    """rows = 3 * 64 + 63: stream 3 would reach past the end."""
    _rejected(lib, b"comet_landmark_update: stream index outside the state", rows=255, streams=[0, 3])


@pytest.mark.parametrize("streams,n", [([2, 2], 2), ([0, 1, 0], 3)])
def test_landmark_update_rejects_two_hops_of_one_stream(lib, streams, n):
    _rejected(lib, b"comet_landmark_update: duplicate stream index", streams=streams, n=n)


@pytest.mark.parametrize("fx,fy", [(0.0, 100.0), (100.0, 0.0), (-100.0, 100.0), (100.0, -1.0), (float("nan"), 100.0),
                                   (100.0, float("nan")), (float("inf"), 100.0), (100.0, float("inf"))])
@pytest.mark.parametrize("hop", [0, 1])
def test_landmark_update_rejects_focal_lengths_that_are_not_finite_and_positive(lib, fx, fy, hop):
    intr = [(100.0, 100.0, 64.0, 64.0)] * 2
    intr[hop] = (fx, fy, 64.0, 64.0)
    _rejected(lib, b"comet_landmark_update: fx and fy must be finite and positive", intr=intr)


@pytest.mark.parametrize("flag", [-1, 2])
def test_landmark_update_rejects_an_unknown_rotation_flag(lib, flag):
    _rejected(lib, b"comet_landmark_update: inverse_rotation must be 0 or 1", inverse_rotation=flag)


@pytest.mark.parametrize("min_obs", [1, 0, -2])
def test_landmark_update_rejects_fewer_than_two_observations(lib, min_obs):
    _rejected(lib, b"comet_landmark_update: min_obs must be at least 2", min_obs=min_obs)


@pytest.mark.parametrize("min_pivot", [-1e-9, 1.0, 2.0, float("nan"), float("inf")])
def test_landmark_update_rejects_a_pivot_bound_outside_0_to_1(lib, min_pivot):
    _rejected(lib, b"comet_landmark_update: min_pivot outside [0, 1)", min_pivot=min_pivot)


@pytest.mark.parametrize("name,shift", [("tracks", 4), ("T", 4), ("intr", 4), ("X", 4), ("R", 8), ("acc", 8)])
def test_landmark_update_rejects_misaligned_point_arrays(lib, name, shift):
    args = _Args()
    args.a[IDX[name]] += shift
    assert _call(lib, args) == -1
    assert b"8-B aligned, R and acc 16-B aligned" in lib.comet_last_error()


def test_landmark_update_checks_in_the_documented_order(lib):
    bad = dict(n=0, N=0, Tw=1, s=0, rows=0, streams=[7, 7], intr=[(0.0, 1.0, 0.0, 0.0)] * 2, inverse_rotation=3,
               min_obs=1, min_pivot=1.0)
    args = _Args(**bad)
    args.a[0] = None
    assert _call(lib, args) == -1 and b"null pointer" in lib.comet_last_error()
    fixes = [("n must be positive", dict(n=2)), ("N outside", dict(N=8)), ("T must be at least 2", dict(Tw=3)),
             ("s outside", dict(s=2)), ("rows below", dict(rows=32)), ("stream index outside", dict(streams=[3, 3])),
             ("duplicate stream", dict(streams=[3, 1])), ("fx and fy", dict(intr=[(5.0, 5.0, 0.0, 0.0)] * 2)),
             ("inverse_rotation", dict(inverse_rotation=1)), ("min_obs", dict(min_obs=2)),
             ("min_pivot", dict(min_pivot=0.0))]
    for message, fix in fixes:
        assert _call(lib, _Args(**bad)) == -1 and message.encode() in lib.comet_last_error(), message
        bad.update(fix)
    args = _Args(**bad)
    args.a[IDX["X"]] += 4
    assert _call(lib, args) == -1 and b"aligned" in lib.comet_last_error()
