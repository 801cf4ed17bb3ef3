"""CPU-side checks of comet_landmark_pnp (csrc/pnp.hip): exported, declared, bound, and every bad
argument is reported through comet_last_error before anything is launched (no GPU needed)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

N_ARGS = 33
NAMES = ["tracks", "weights", "X", "state", "R0", "T0", "intr", "intr_host", "n", "Tw", "N", "s", "inverse_rotation",
         "iters", "huber_px", "min_pts", "min_pivot", "fuse_acc", "rows", "slots", "slots_host", "inject_w", "fuse_fx",
         "fuse_fy", "fuse_cx", "fuse_cy", "q_out", "R_out", "t_out", "n_in", "rms_px", "state_out"]
IDX = {name: i for i, name in enumerate(NAMES)}
SCALARS = ("n", "Tw", "N", "s", "inverse_rotation", "iters", "huber_px", "min_pts", "min_pivot", "rows", "inject_w",
           "fuse_fx", "fuse_fy", "fuse_cx", "fuse_cy")
POINTERS = [i for i, name in enumerate(NAMES) if name not in SCALARS]
OPTIONAL = ("weights", "fuse_acc", "slots", "slots_host")


@pytest.fixture(scope="module")
def lib():
    from comet_amd import _lib
    return _lib.load()


class _Args:
    """Well-formed arguments over host memory (rejected calls never read the device pointers)."""

    def __init__(self, slots=None, intr=None, inject=True, **kw):
        self.buf = ctypes.create_string_buffer(1 << 14)
        base = ctypes.addressof(self.buf) + (-ctypes.addressof(self.buf)) % 256
        p = {name: base + 512 * k for k, name in enumerate(NAMES[i] for i in POINTERS)}
        v = dict(n=2, Tw=4, N=64, s=1, inverse_rotation=0, iters=4, huber_px=3.0, min_pts=6, min_pivot=1e-8, rows=16,
                 inject_w=1.0, fuse_fx=100.0, fuse_fy=100.0, fuse_cx=64.0, fuse_cy=64.0)
        v.update(kw)
        n = max(v["n"], 1)
        slots = list(range(n * max(v["Tw"], 1))) if slots is None else slots
        intr = [(100.0, 110.0, 64.0, 64.0)] * n if intr is None else intr
        self.slots = (ctypes.c_int32 * len(slots))(*slots)
        flat = [x for row in intr for x in row]
        self.intr = (ctypes.c_double * len(flat))(*flat)
        p["slots_host"], p["intr_host"] = ctypes.addressof(self.slots), ctypes.addressof(self.intr)
        if not inject:
            p["fuse_acc"] = p["slots"] = p["slots_host"] = None
        self.a = [p[name] if name in p else v[name] for name in NAMES] + [None]
        assert len(self.a) == N_ARGS


def _call(lib, args):
    return lib.comet_landmark_pnp(*args.a)


def _rejected(lib, message, **kw):
    assert _call(lib, _Args(**kw)) == -1
    assert message in lib.comet_last_error(), lib.comet_last_error()


def test_landmark_pnp_is_exported_declared_and_bound(lib):
    from comet_amd import _lib
    src = open(os.path.join(ROOT, "include", "comet_hip.h")).read()
    m = re.search(r"^\s*int\s+comet_landmark_pnp\((.*?)\);", src, re.M | re.S)
    assert m, "comet_landmark_pnp is not declared in include/comet_hip.h"
    params = [a.strip() for a in m.group(1).split(",")]
    assert "comet_landmark_pnp" in _lib.SIGNATURES, "comet_landmark_pnp is not bound in comet_amd._lib"
    res, argtypes = _lib.SIGNATURES["comet_landmark_pnp"]
    assert res is ctypes.c_int and len(params) == len(argtypes) == N_ARGS
    for prm, ty in zip(params, argtypes):
        if "*" in prm:
            assert ty is ctypes.c_void_p, prm
        elif prm.startswith("double"):
            assert ty is ctypes.c_double, prm
        else:
            assert prm.startswith("int ") and ty is ctypes.c_int, prm
    assert hasattr(lib, "comet_landmark_pnp")
    assert [p.split()[-1].lstrip("*") for p in params[:32]] == NAMES
    assert re.search(r"#define\s+COMET_PNP_MAX_ITERS\s+16\b", src) and _lib.PNP_MAX_ITERS == 16
    # csrc/*.hip is the Makefile's source list: the kernel's file is part of the library
    mk = open(os.path.join(ROOT, "comet-pose-estimation_amd", "Makefile")).read()
    assert "$(wildcard csrc/*.hip)" in mk
    assert os.path.isfile(os.path.join(ROOT, "comet-pose-estimation_amd", "csrc", "pnp.hip"))


@pytest.mark.parametrize("index", [i for i in POINTERS if NAMES[i] not in OPTIONAL])
def test_landmark_pnp_rejects_null_pointers(lib, index):
    args = _Args()
    args.a[index] = None
    assert _call(lib, args) == -1
    assert b"comet_landmark_pnp: null pointer" in lib.comet_last_error()


@pytest.mark.parametrize("name", ["slots", "slots_host"])
def test_landmark_pnp_rejects_an_accumulator_without_its_slot_tables(lib, name):
    args = _Args()
    args.a[IDX[name]] = None
    assert _call(lib, args) == -1
    assert b"comet_landmark_pnp: null pointer" in lib.comet_last_error()


def test_landmark_pnp_optional_pointers_pass_the_pointer_check(lib):
    """weights may be null, and fuse_acc with its slot tables: with them null and a bad n, the report is about n."""
    args = _Args(n=0, inject=False)
    args.a[IDX["weights"]] = None
    assert _call(lib, args) == -1
    assert b"comet_landmark_pnp: n must be positive" in lib.comet_last_error()


@pytest.mark.parametrize("n", [0, -1])
def test_landmark_pnp_rejects_nonpositive_n(lib, n):
    _rejected(lib, b"comet_landmark_pnp: n must be positive", n=n)


@pytest.mark.parametrize("N", [0, -5, 4097, 1 << 30])
def test_landmark_pnp_rejects_track_counts_outside_1_to_4096(lib, N):
    _rejected(lib, b"comet_landmark_pnp: N outside [1, 4096]", N=N)


@pytest.mark.parametrize("T", [1, 0, -3])
def test_landmark_pnp_rejects_windows_below_two_frames(lib, T):
    _rejected(lib, b"comet_landmark_pnp: T must be at least 2", Tw=T, s=1)


@pytest.mark.parametrize("s,T", [(0, 4), (4, 4), (-1, 4), (7, 4), (2, 2)])
def test_landmark_pnp_rejects_a_stride_outside_the_window(lib, s, T):
    _rejected(lib, b"comet_landmark_pnp: s outside [1, T - 1]", s=s, Tw=T)


@pytest.mark.parametrize("iters", [0, -1, 17, 1 << 20])
def test_landmark_pnp_rejects_iteration_counts_outside_1_to_16(lib, iters):
    _rejected(lib, b"comet_landmark_pnp: iters outside [1, 16]", iters=iters)


@pytest.mark.parametrize("huber", [0.0, -1.0, float("nan"), float("inf")])
def test_landmark_pnp_rejects_a_huber_threshold_that_is_not_finite_and_positive(lib, huber):
    _rejected(lib, b"comet_landmark_pnp: huber_px must be finite and positive", huber_px=huber)


@pytest.mark.parametrize("min_pts", [3, 0, -2])
def test_landmark_pnp_rejects_fewer_than_four_points(lib, min_pts):
    _rejected(lib, b"comet_landmark_pnp: min_pts must be at least 4", min_pts=min_pts)


@pytest.mark.parametrize("min_pivot", [-1e-9, 1.0, 2.0, float("nan"), float("inf")])
def test_landmark_pnp_rejects_a_pivot_bound_outside_0_to_1(lib, min_pivot):
    _rejected(lib, b"comet_landmark_pnp: min_pivot outside [0, 1)", min_pivot=min_pivot)


@pytest.mark.parametrize("flag", [-1, 2])
def test_landmark_pnp_rejects_an_unknown_rotation_flag(lib, flag):
    _rejected(lib, b"comet_landmark_pnp: inverse_rotation must be 0 or 1", inverse_rotation=flag)


@pytest.mark.parametrize("fx,fy", [(0.0, 100.0), (100.0, 0.0), (-100.0, 100.0), (100.0, -1.0), (float("nan"), 100.0),
                                   (100.0, float("nan")), (float("inf"), 100.0), (100.0, float("inf"))])
@pytest.mark.parametrize("hop", [0, 1])
def test_landmark_pnp_rejects_focal_lengths_that_are_not_finite_and_positive(lib, fx, fy, hop):
    intr = [(100.0, 100.0, 64.0, 64.0)] * 2
    intr[hop] = (fx, fy, 64.0, 64.0)
    _rejected(lib, b"comet_landmark_pnp: fx and fy must be finite and positive", intr=intr)


@pytest.mark.parametrize("w", [-1.0, float("nan"), float("inf")])
def test_landmark_pnp_rejects_an_injection_weight_that_is_not_finite_or_negative(lib, w):
    _rejected(lib, b"comet_landmark_pnp: inject_w must be finite and >= 0", inject_w=w)


@pytest.mark.parametrize("slots", [[0, 1, 2, 3, 4, 5, 6, 16], [-1, 1, 2, 3, 4, 5, 6, 7], [1 << 20] + list(range(7))])
def test_landmark_pnp_rejects_slots_outside_the_ring(lib, slots):
    _rejected(lib, b"comet_landmark_pnp: slot index outside the ring", slots=slots)  # rows = 16


@pytest.mark.parametrize("slots", [[0, 1, 2, 3, 4, 5, 6, 0], [3, 3, 2, 1, 4, 5, 6, 7]])
def test_landmark_pnp_rejects_two_positions_on_one_row(lib, slots):
    _rejected(lib, b"comet_landmark_pnp: duplicate slot index", slots=slots)


def test_landmark_pnp_without_an_accumulator_skips_the_injection_checks(lib):
    """No fuse_acc: inject_w, rows and the slot tables are not looked at; the next report is the alignment's."""
    args = _Args(inject=False, inject_w=float("nan"), rows=-3)
    args.a[IDX["X"]] += 4
    assert _call(lib, args) == -1 and b"aligned" in lib.comet_last_error()


@pytest.mark.parametrize("name,shift", [("tracks", 4), ("X", 4), ("T0", 4), ("intr", 4), ("q_out", 4), ("t_out", 4),
                                        ("R0", 8), ("fuse_acc", 8)])
def test_landmark_pnp_rejects_misaligned_arrays(lib, name, shift):
    args = _Args()
    args.a[IDX[name]] += shift
    assert _call(lib, args) == -1
    assert b"8-B aligned, R0 and fuse_acc 16-B aligned" in lib.comet_last_error()


def test_landmark_pnp_checks_in_the_documented_order(lib):
    bad = dict(n=0, N=0, Tw=1, s=0, iters=0, huber_px=0.0, min_pts=3, min_pivot=1.0, inverse_rotation=3,
               intr=[(0.0, 1.0, 0.0, 0.0)] * 2, inject_w=-1.0, slots=[40, 40, 0, 1, 2, 3], rows=8)
    args = _Args(**bad)
    args.a[0] = None
    assert _call(lib, args) == -1 and b"null pointer" in lib.comet_last_error()
    fixes = [("n must be positive", dict(n=2)), ("N outside", dict(N=8)), ("T must be at least 2", dict(Tw=3)),
             ("s outside", dict(s=2)), ("iters outside", dict(iters=16)), ("huber_px", dict(huber_px=1e-3)),
             ("min_pts", dict(min_pts=4)), ("min_pivot", dict(min_pivot=0.0)),
             ("inverse_rotation", dict(inverse_rotation=1)), ("fx and fy", dict(intr=[(5.0, 5.0, 0.0, 0.0)] * 2)),
             ("inject_w", dict(inject_w=0.0)), ("slot index outside", dict(slots=[7, 7, 0, 1, 2, 3])),
             ("duplicate slot", dict(slots=[7, 6, 0, 1, 2, 3]))]
    for message, fix in fixes:
        assert _call(lib, _Args(**bad)) == -1 and message.encode() in lib.comet_last_error(), message
        bad.update(fix)
    args = _Args(**bad)
    args.a[IDX["X"]] += 4
    assert _call(lib, args) == -1 and b"aligned" in lib.comet_last_error()
