"""CPU-side checks of comet_landmark_reid (csrc/reid.hip): exported, declared, bound, and every bad argument
is reported through comet_last_error before anything is launched, in the documented order (no GPU needed)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

N_ARGS = 33
NAMES = ["tracks", "R", "T", "ids", "src", "stream_idx", "stream_idx_host", "intr", "intr_host", "acc", "acc_id", "alias",
         "rows", "arch", "arch_id", "arch_cursor", "entries", "ws", "n", "Tw", "N", "C", "inverse_rotation",
         "arch_min_obs", "min_pivot", "reid_px", "reid_min_cos", "src_lm", "lm_id", "reid_state", "reid_dist", "stats"]
IDX = {name: i for i, name in enumerate(NAMES)}
SCALARS = ("rows", "entries", "n", "Tw", "N", "C", "inverse_rotation", "arch_min_obs", "min_pivot", "reid_px",
           "reid_min_cos")
POINTERS = [i for i, name in enumerate(NAMES) if name not in SCALARS]


@pytest.fixture(scope="module")
def lib():
    from comet_amd import _lib
    return _lib.load()


class _Args:
    """Well-formed arguments over host memory (rejected calls never read the device pointers)."""

    def __init__(self, streams=None, intr=None, **kw):
        self.buf = ctypes.create_string_buffer(1 << 15)
        base = ctypes.addressof(self.buf) + (-ctypes.addressof(self.buf)) % 256
        p = {name: base + 512 * k for k, name in enumerate(NAMES[i] for i in POINTERS)}
        v = dict(rows=4 * 64, entries=4 * 32, n=2, Tw=4, N=64, C=32, inverse_rotation=0, arch_min_obs=3, min_pivot=1e-8,
                 reid_px=2.0, reid_min_cos=0.5)
        v.update(kw)
        n = max(v["n"], 1)
        streams = list(range(n)) if streams is None else streams
        intr = [300.0, 310.0, 63.5, 60.0] * n if intr is None else intr
        self.streams = (ctypes.c_int32 * len(streams))(*streams)
        self.intr = (ctypes.c_double * len(intr))(*intr)
        p["stream_idx_host"], p["intr_host"] = ctypes.addressof(self.streams), ctypes.addressof(self.intr)
        self.a = [p[name] if name in p else v[name] for name in NAMES] + [None]
        assert len(self.a) == N_ARGS


def _call(lib, args):
    return lib.comet_landmark_reid(*args.a)


def _rejected(lib, message, **kw):
    assert _call(lib, _Args(**kw)) == -1
    assert message in lib.comet_last_error(), lib.comet_last_error()


def test_landmark_reid_is_exported_declared_and_bound(lib):
    from comet_amd import _lib, ops
    src = open(os.path.join(ROOT, "include", "comet_hip.h")).read()
    m = re.search(r"^\s*int\s+comet_landmark_reid\((.*?)\);", src, re.M | re.S)
    assert m, "comet_landmark_reid is not declared in include/comet_hip.h"
    params = [a.strip() for a in m.group(1).split(",")]
    assert "comet_landmark_reid" in _lib.SIGNATURES, "comet_landmark_reid is not bound in comet_amd._lib"
    res, argtypes = _lib.SIGNATURES["comet_landmark_reid"]
    assert res is ctypes.c_int and len(params) == len(argtypes) == N_ARGS
    for prm, ty in zip(params, argtypes):
        if "*" in prm:
            assert ty is ctypes.c_void_p, prm
        elif prm.startswith("double"):
            assert ty is ctypes.c_double, prm
        else:
            assert prm.startswith("int ") and ty is ctypes.c_int, prm
    assert hasattr(lib, "comet_landmark_reid")
    assert [p.split()[-1].lstrip("*") for p in params[:32]] == NAMES
    assert re.search(r"#define\s+COMET_LM_ARCH_ROW\s+20\b", src) and _lib.LM_ARCH_ROW == 20
    assert re.search(r"#define\s+COMET_LM_ARCH_MAX\s+4096\b", src) and _lib.LM_ARCH_MAX == 4096
    assert ops.ReidOut._fields == ("src_lm", "lm_id", "reid_state", "reid_dist", "stats") and callable(ops.landmark_reid)


@pytest.mark.parametrize("index", POINTERS)
def test_landmark_reid_rejects_null_pointers(lib, index):
    args = _Args()
    args.a[index] = None
    assert _call(lib, args) == -1
    assert b"comet_landmark_reid: null pointer" in lib.comet_last_error()


@pytest.mark.parametrize("n", [0, -1])
def test_landmark_reid_rejects_nonpositive_n(lib, n):
    _rejected(lib, b"comet_landmark_reid: n must be positive", n=n)


@pytest.mark.parametrize("N", [0, -1, 4097])
def test_landmark_reid_rejects_track_counts_outside_1_to_4096(lib, N):
    _rejected(lib, b"comet_landmark_reid: N outside [1, 4096]", N=N)


@pytest.mark.parametrize("C", [0, -1, 4097])
def test_landmark_reid_rejects_capacities_outside_1_to_4096(lib, C):
    _rejected(lib, b"comet_landmark_reid: C outside [1, 4096]", C=C)


@pytest.mark.parametrize("T", [1, 0, -3])
def test_landmark_reid_rejects_windows_below_two_frames(lib, T):
    _rejected(lib, b"comet_landmark_reid: T must be at least 2", Tw=T)


def test_landmark_reid_rejects_a_state_too_small_for_the_hops(lib):
    _rejected(lib, b"comet_landmark_reid: rows below n * N", rows=2 * 64 - 1)
    _rejected(lib, b"comet_landmark_reid: entries below n * C", entries=2 * 32 - 1)


@pytest.mark.parametrize("streams", [[0, 4], [-1, 0], [4, 5], [1 << 20, 0]])
def test_landmark_reid_rejects_stream_indices_outside_the_state(lib, streams):
    _rejected(lib, b"comet_landmark_reid: stream index outside the state", streams=streams)  # S = 4


def test_landmark_reid_takes_the_smaller_of_the_two_stream_counts(lib):
    _rejected(lib, b"comet_landmark_reid: stream index outside the state", streams=[0, 3], entries=3 * 32)
    _rejected(lib, b"comet_landmark_reid: stream index outside the state", streams=[0, 3], rows=3 * 64)


@pytest.mark.parametrize("streams,n", [([2, 2], 2), ([0, 1, 0], 3)])
def test_landmark_reid_rejects_two_hops_of_one_stream(lib, streams, n):
    _rejected(lib, b"comet_landmark_reid: duplicate stream index", streams=streams, n=n)


@pytest.mark.parametrize("k,value", [(0, 0.0), (0, -1.0), (0, float("nan")), (0, float("inf")), (5, 0.0), (5, float("nan"))])
def test_landmark_reid_rejects_bad_focal_lengths(lib, k, value):
    intr = [300.0, 310.0, 63.5, 60.0] * 2
    intr[k] = value
    _rejected(lib, b"comet_landmark_reid: fx and fy must be finite and positive", intr=intr)


@pytest.mark.parametrize("flag", [-1, 2])
def test_landmark_reid_rejects_an_unknown_rotation_flag(lib, flag):
    _rejected(lib, b"comet_landmark_reid: inverse_rotation must be 0 or 1", inverse_rotation=flag)


@pytest.mark.parametrize("m", [1, 0, -2])
def test_landmark_reid_rejects_fewer_than_two_observations(lib, m):
    _rejected(lib, b"comet_landmark_reid: arch_min_obs must be at least 2", arch_min_obs=m)


@pytest.mark.parametrize("p", [-1e-9, 1.0, 2.0, float("nan")])
def test_landmark_reid_rejects_a_pivot_bound_outside_0_to_1(lib, p):
    _rejected(lib, b"comet_landmark_reid: min_pivot outside [0, 1)", min_pivot=p)


@pytest.mark.parametrize("px", [0.0, -1.0, float("nan"), float("inf")])
def test_landmark_reid_rejects_a_gate_that_is_not_finite_and_positive(lib, px):
    _rejected(lib, b"comet_landmark_reid: reid_px must be finite and positive", reid_px=px)


@pytest.mark.parametrize("c", [-1.0001, 1.0001, float("nan"), float("inf")])
def test_landmark_reid_rejects_a_cosine_outside_minus_1_to_1(lib, c):
    _rejected(lib, b"comet_landmark_reid: reid_min_cos outside [-1, 1]", reid_min_cos=c)


@pytest.mark.parametrize("name,shift", [("tracks", 4), ("T", 4), ("intr", 4), ("R", 8), ("acc", 8), ("arch", 8), ("ws", 8)])
def test_landmark_reid_rejects_misaligned_arrays(lib, name, shift):
    args = _Args()
    args.a[IDX[name]] += shift
    assert _call(lib, args) == -1
    assert b"tracks, T and intr must be 8-B aligned, R, acc, arch and ws 16-B aligned" in lib.comet_last_error()


def test_landmark_reid_checks_in_the_documented_order(lib):
    bad = dict(n=0, N=0, C=0, Tw=1, rows=0, entries=0, streams=[7, 7], intr=[0.0, 1.0, 0.0, 0.0] * 2, inverse_rotation=3,
               arch_min_obs=1, min_pivot=1.0, reid_px=0.0, reid_min_cos=2.0)
    args = _Args(**bad)
    args.a[0] = None
    assert _call(lib, args) == -1 and b"null pointer" in lib.comet_last_error()
    fixes = [("n must be positive", dict(n=2)), ("N outside", dict(N=64)), ("C outside", dict(C=32)),
             ("T must be at least 2", dict(Tw=3)), ("rows below", dict(rows=4 * 64)), ("entries below", dict(entries=4 * 32)),
             ("stream index outside", dict(streams=[3, 3])), ("duplicate stream", dict(streams=[3, 1])),
             ("fx and fy", dict(intr=[300.0, 310.0, 0.0, 0.0] * 2)), ("inverse_rotation", dict(inverse_rotation=1)),
             ("arch_min_obs", dict(arch_min_obs=2)), ("min_pivot outside", dict(min_pivot=0.0)),
             ("reid_px", dict(reid_px=1.5)), ("reid_min_cos", dict(reid_min_cos=-1.0))]
    for message, fix in fixes:
        assert _call(lib, _Args(**bad)) == -1 and message.encode() in lib.comet_last_error(), message
        bad.update(fix)
    args = _Args(**bad)
    args.a[IDX["ws"]] += 8
    assert _call(lib, args) == -1 and b"aligned" in lib.comet_last_error()
