"""CPU-side checks of comet_track_carry (csrc/carry.hip): exported, declared, bound, and every bad
argument is reported through comet_last_error before anything is launched (no GPU needed)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

N_ARGS = 25
# tracks, score, ids, age, mask, cand, cand_n, next_id, prev_valid, n, T, N, M, s, H, W, cell, border,
# min_score, query, ids_out, age_out, src, stats, stream
IDX = {"mask": 4, "cand": 5, "n": 9, "T": 10, "N": 11, "M": 12, "s": 13, "H": 14, "W": 15, "cell": 16, "border": 17}


@pytest.fixture(scope="module")
def lib():
    from comet_amd import _lib
    return _lib.load()


class _Args:
    """Well-formed arguments over host memory (rejected calls never read the device pointers)."""

    def __init__(self, **kw):
        self.buf = ctypes.create_string_buffer(1 << 14)
        base = ctypes.addressof(self.buf) + (-ctypes.addressof(self.buf)) % 256
        p = [base + 512 * k for k in range(20)]
        v = dict(n=2, T=4, N=64, M=96, s=1, H=128, W=128, cell=8, border=0)
        v.update(kw)
        self.a = [p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], v["n"], v["T"], v["N"], v["M"], v["s"], v["H"],
                  v["W"], v["cell"], v["border"], 0.5, p[9], p[10], p[11], p[12], p[13], None]
        assert len(self.a) == N_ARGS


def _call(lib, args):
    return lib.comet_track_carry(*args.a)


def _rejected(lib, message, **kw):
    assert _call(lib, _Args(**kw)) == -1
    assert message in lib.comet_last_error(), lib.comet_last_error()


def test_track_carry_is_exported_declared_and_bound(lib):
    from comet_amd import _lib
    src = open(os.path.join(ROOT, "include", "comet_hip.h")).read()
    m = re.search(r"^\s*int\s+comet_track_carry\((.*?)\);", src, re.M | re.S)
    assert m, "comet_track_carry is not declared in include/comet_hip.h"
    params = [a.strip() for a in m.group(1).split(",")]
    res, argtypes = _lib.SIGNATURES["comet_track_carry"]
    assert res is ctypes.c_int and len(params) == len(argtypes) == N_ARGS
    for prm, ty in zip(params, argtypes):
        if "*" in prm:
            assert ty is ctypes.c_void_p, prm
        elif prm.startswith("float"):
            assert ty is ctypes.c_float, prm
        else:
            assert prm.startswith("int ") and ty is ctypes.c_int, prm
    assert hasattr(lib, "comet_track_carry")
    for name, value in (("TRACKS", 4096), ("CANDIDATES", 65536), ("CELLS", 8192)):
        assert re.search(rf"#define\s+COMET_CARRY_MAX_{name}\s+{value}\b", src)
        assert getattr(_lib, f"CARRY_MAX_{name}") == value


# the pointers that must not be null: everything but mask (4), cand (5: its own message) and the stream (24)
@pytest.mark.parametrize("index", [0, 1, 2, 3, 6, 7, 8, 19, 20, 21, 22, 23])
def test_track_carry_rejects_null_pointers(lib, index):
    args = _Args()
    args.a[index] = None
    assert _call(lib, args) == -1
    assert b"comet_track_carry: null pointer" in lib.comet_last_error()


def test_track_carry_cand_may_be_null_only_without_candidates(lib):
    args = _Args()
    args.a[IDX["cand"]] = None
    assert _call(lib, args) == -1
    assert b"comet_track_carry: cand may be null only when M is 0" in lib.comet_last_error()


@pytest.mark.parametrize("n", [0, -1])
def test_track_carry_rejects_nonpositive_n(lib, n):
    _rejected(lib, b"comet_track_carry: n must be positive", n=n)


@pytest.mark.parametrize("N", [0, -5, 4097, 1 << 30])
def test_track_carry_rejects_track_counts_outside_1_to_4096(lib, N):
    _rejected(lib, b"comet_track_carry: N outside [1, 4096]", N=N)


@pytest.mark.parametrize("M", [-1, 65537, 1 << 30])
def test_track_carry_rejects_candidate_counts_outside_0_to_65536(lib, M):
    _rejected(lib, b"comet_track_carry: M outside [0, 65536]", M=M)


@pytest.mark.parametrize("s,T", [(0, 4), (4, 4), (-1, 4), (1, 1), (7, 4), (1, 0)])
def test_track_carry_rejects_a_row_outside_the_window(lib, s, T):
    _rejected(lib, b"comet_track_carry: s outside [1, T - 1]", s=s, T=T)


@pytest.mark.parametrize("H,W", [(0, 128), (128, 0), (-4, 128), (128, -1)])
def test_track_carry_rejects_empty_frames(lib, H, W):
    _rejected(lib, b"comet_track_carry: H and W must be positive", H=H, W=W)


@pytest.mark.parametrize("cell", [0, -8])
def test_track_carry_rejects_cells_below_one_pixel(lib, cell):
    _rejected(lib, b"comet_track_carry: cell must be at least 1", cell=cell)


def test_track_carry_rejects_a_negative_border(lib):
    _rejected(lib, b"comet_track_carry: negative border", border=-1)


@pytest.mark.parametrize("H,W,cell", [(128, 128, 1), (728, 728, 8), (91, 91, 1), (1 << 20, 1 << 20, 8)])
def test_track_carry_rejects_more_than_8192_cells(lib, H, W, cell):
    """128 x 128 cells of 1 px, 91 x 91 (8281) cells; 90 x 91 = 8190 cells pass this check."""
    _rejected(lib, b"comet_track_carry: more than 8192 grid cells", H=H, W=W, cell=cell)


def test_track_carry_rejects_misaligned_points(lib):
    args = _Args()
    args.a[0] += 4
    assert _call(lib, args) == -1
    assert b"comet_track_carry: tracks, cand and query must be 8-B aligned" in lib.comet_last_error()


def test_track_carry_checks_in_the_documented_order(lib):
    """Everything wrong at once: the null pointer is reported; with pointers, n; then N."""
    bad = dict(n=0, N=0, M=-1, s=0, H=0, cell=0, border=-1)
    args = _Args(**bad)
    args.a[0] = None
    assert _call(lib, args) == -1 and b"null pointer" in lib.comet_last_error()
    assert _call(lib, _Args(**bad)) == -1 and b"n must be positive" in lib.comet_last_error()
    assert _call(lib, _Args(**dict(bad, n=1))) == -1 and b"N outside" in lib.comet_last_error()
