"""CPU-side checks of comet_motion_fit (csrc/motion.hip): exported, declared, bound, and every bad
argument is reported through comet_last_error before anything is launched, in the documented order (no
GPU needed)."""
import ctypes
import math
import os
import re

import pytest

from conftest import ROOT

N_ARGS = 32
NAMES = ["R", "T", "weights", "first", "stream_idx", "stream_idx_host", "hist", "hist_n", "S", "cap", "n", "Tw", "s",
         "fit_len", "min_frames", "iters", "horizon", "max_angle", "inverse_rotation", "omega", "q0", "vel", "t0",
         "rot_rms", "trans_rms", "n_used", "state", "pred_q", "pred_t", "innov_rot", "innov_trans"]
IDX = {name: i for i, name in enumerate(NAMES)}
SCALARS = ("S", "cap", "n", "Tw", "s", "fit_len", "min_frames", "iters", "horizon", "max_angle", "inverse_rotation")
POINTERS = [i for i, name in enumerate(NAMES) if name not in SCALARS]


@pytest.fixture(scope="module")
def lib():
    from comet_amd import _lib
    return _lib.load()


class _Args:
    """Well-formed arguments over host memory (rejected calls never read the device pointers)."""

    def __init__(self, streams=None, **kw):
        self.buf = ctypes.create_string_buffer(1 << 15)
        base = ctypes.addressof(self.buf) + (-ctypes.addressof(self.buf)) % 256
        p = {name: base + 512 * k for k, name in enumerate(NAMES[i] for i in POINTERS)}
        v = dict(S=4, cap=16, n=2, Tw=4, s=1, fit_len=16, min_frames=3, iters=2, horizon=1, max_angle=2.0,
                 inverse_rotation=0)
        v.update(kw)
        streams = list(range(max(v["n"], 1))) if streams is None else streams
        self.streams = (ctypes.c_int32 * len(streams))(*streams)
        p["stream_idx_host"] = ctypes.addressof(self.streams)
        self.a = [p[name] if name in p else v[name] for name in NAMES] + [None]
        assert len(self.a) == N_ARGS


def _call(lib, args):
    return lib.comet_motion_fit(*args.a)


def _rejected(lib, message, **kw):
    assert _call(lib, _Args(**kw)) == -1
    assert message in lib.comet_last_error(), lib.comet_last_error()


def test_motion_fit_is_exported_declared_and_bound(lib):
    from comet_amd import _lib
    src = open(os.path.join(ROOT, "include", "comet_hip.h")).read()
    m = re.search(r"^\s*int\s+comet_motion_fit\((.*?)\);", src, re.M | re.S)
    assert m, "comet_motion_fit is not declared in include/comet_hip.h"
    params = [a.strip() for a in m.group(1).split(",")]
    assert "comet_motion_fit" in _lib.SIGNATURES, "comet_motion_fit is not bound in comet_amd._lib"
    res, argtypes = _lib.SIGNATURES["comet_motion_fit"]
    assert res is ctypes.c_int and len(params) == len(argtypes) == N_ARGS
    for prm, ty in zip(params, argtypes):
        if "*" in prm:
            assert ty is ctypes.c_void_p, prm
        elif prm.startswith("double"):
            assert ty is ctypes.c_double, prm
        else:
            assert prm.startswith("int ") and ty is ctypes.c_int, prm
    assert hasattr(lib, "comet_motion_fit")
    assert [p.split()[-1].lstrip("*") for p in params[:31]] == NAMES
    assert re.search(r"#define\s+COMET_MOTION_ROW\s+8\b", src) and _lib.MOTION_ROW == 8
    assert re.search(r"#define\s+COMET_MOTION_MAX_ITERS\s+8\b", src) and _lib.MOTION_MAX_ITERS == 8
    assert re.search(r"#define\s+COMET_MOTION_MAX_HORIZON\s+64\b", src) and _lib.MOTION_MAX_HORIZON == 64
    assert re.search(r"#define\s+COMET_MOTION_COUNT_FOLD\s+\(1 << 30\)", src) and _lib.MOTION_COUNT_FOLD == 1 << 30


# the pointers that must not be null: everything but weights (2) and the stream (31)
@pytest.mark.parametrize("index", [i for i in POINTERS if i != 2])
def test_motion_fit_rejects_null_pointers(lib, index):
    args = _Args()
    args.a[index] = None
    assert _call(lib, args) == -1
    assert b"comet_motion_fit: null pointer" in lib.comet_last_error()


def test_motion_fit_null_weights_pass_the_pointer_check(lib):
    """weights may be null: with null weights and a bad n, the report is about n."""
    args = _Args(n=0)
    args.a[IDX["weights"]] = None
    assert _call(lib, args) == -1
    assert b"comet_motion_fit: n must be positive" in lib.comet_last_error()


@pytest.mark.parametrize("n", [0, -1])
def test_motion_fit_rejects_nonpositive_n(lib, n):
    _rejected(lib, b"comet_motion_fit: n must be positive", n=n)


@pytest.mark.parametrize("T", [1, 0, -3])
def test_motion_fit_rejects_windows_below_two_frames(lib, T):
    _rejected(lib, b"comet_motion_fit: T must be at least 2", Tw=T, s=1)


@pytest.mark.parametrize("s,T", [(0, 4), (4, 4), (-1, 4), (7, 4), (2, 2)])
def test_motion_fit_rejects_a_stride_outside_the_window(lib, s, T):
    _rejected(lib, b"comet_motion_fit: s outside [1, T - 1]", s=s, Tw=T)


@pytest.mark.parametrize("cap", [1, 0, -4, 65, 1 << 20])
def test_motion_fit_rejects_a_ring_outside_2_to_64(lib, cap):
    _rejected(lib, b"comet_motion_fit: cap outside [2, 64]", cap=cap, fit_len=2)


@pytest.mark.parametrize("fit_len,cap", [(1, 16), (0, 16), (17, 16), (64, 63)])
def test_motion_fit_rejects_a_fit_length_outside_2_to_cap(lib, fit_len, cap):
    _rejected(lib, b"comet_motion_fit: fit_len outside [2, cap]", fit_len=fit_len, cap=cap, min_frames=2)


@pytest.mark.parametrize("min_frames,fit_len", [(1, 16), (0, 16), (17, 16), (3, 2)])
def test_motion_fit_rejects_min_frames_outside_2_to_fit_len(lib, min_frames, fit_len):
    _rejected(lib, b"comet_motion_fit: min_frames outside [2, fit_len]", min_frames=min_frames, fit_len=fit_len)


@pytest.mark.parametrize("iters", [0, -1, 9])
def test_motion_fit_rejects_iterations_outside_1_to_8(lib, iters):
    _rejected(lib, b"comet_motion_fit: iters outside [1, 8]", iters=iters)


@pytest.mark.parametrize("horizon", [-1, 65])
def test_motion_fit_rejects_a_horizon_outside_0_to_64(lib, horizon):
    _rejected(lib, b"comet_motion_fit: horizon outside [0, 64]", horizon=horizon)


@pytest.mark.parametrize("max_angle", [0.0, -1.0, math.pi, 4.0, float("nan"), float("inf")])
def test_motion_fit_rejects_an_angle_bound_outside_0_to_pi(lib, max_angle):
    _rejected(lib, b"comet_motion_fit: max_angle outside (0, pi)", max_angle=max_angle)


@pytest.mark.parametrize("flag", [-1, 2])
def test_motion_fit_rejects_an_unknown_rotation_flag(lib, flag):
    _rejected(lib, b"comet_motion_fit: inverse_rotation must be 0 or 1", inverse_rotation=flag)


@pytest.mark.parametrize("streams", [[0, 4], [-1, 0], [4, 5], [1 << 20, 0]])
def test_motion_fit_rejects_stream_indices_outside_the_state(lib, streams):
    _rejected(lib, b"comet_motion_fit: stream index outside the state", streams=streams)  # S = 4


def test_motion_fit_rejects_every_stream_of_an_empty_state(lib):
    _rejected(lib, b"comet_motion_fit: stream index outside the state", S=0)


@pytest.mark.parametrize("streams,n", [([2, 2], 2), ([0, 1, 0], 3)])
def test_motion_fit_rejects_two_hops_of_one_stream(lib, streams, n):
    _rejected(lib, b"comet_motion_fit: duplicate stream index", streams=streams, n=n)


@pytest.mark.parametrize("name,shift", [("R", 8), ("hist", 8), ("T", 4), ("omega", 4), ("q0", 4), ("vel", 4), ("t0", 4),
                                        ("pred_q", 4), ("pred_t", 4)])
def test_motion_fit_rejects_misaligned_arrays(lib, name, shift):
    args = _Args()
    args.a[IDX[name]] += shift
    assert _call(lib, args) == -1
    assert b"R and hist must be 16-B aligned, T and the f64 outputs 8-B aligned" in lib.comet_last_error()


def test_motion_fit_checks_in_the_documented_order(lib):
    bad = dict(n=0, Tw=1, s=0, cap=1, fit_len=1, min_frames=1, iters=0, horizon=-1, max_angle=0.0, inverse_rotation=3,
               streams=[7, 7])
    args = _Args(**bad)
    args.a[0] = None
    assert _call(lib, args) == -1 and b"null pointer" in lib.comet_last_error()
    fixes = [("n must be positive", dict(n=2)), ("T must be at least 2", dict(Tw=3)), ("s outside", dict(s=2)),
             ("cap outside", dict(cap=8)), ("fit_len outside", dict(fit_len=8)), ("min_frames outside", dict(min_frames=8)),
             ("iters outside", dict(iters=8)), ("horizon outside", dict(horizon=64)), ("max_angle outside", dict(max_angle=3.0)),
             ("inverse_rotation", dict(inverse_rotation=1)), ("stream index outside", dict(streams=[3, 3])),
             ("duplicate stream", dict(streams=[3, 1]))]
    for message, fix in fixes:
        assert _call(lib, _Args(**bad)) == -1 and message.encode() in lib.comet_last_error(), message
        bad.update(fix)
    args = _Args(**bad)
    args.a[IDX["pred_t"]] += 4
    assert _call(lib, args) == -1 and b"aligned" in lib.comet_last_error()
