"""CPU-side checks of the SIFT entry points of libcomet_hip.so: declared, exported, and bad
arguments rejected on the host before anything is launched."""
import ctypes
import os
import re

from conftest import ROOT

NAMES = ["comet_sift_base", "comet_gauss_blur", "comet_downsample2", "comet_sift_detect"]


def _ptr():
    buf = ctypes.create_string_buffer(1 << 12)
    return buf, ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256  # aligned host address (never read)


def test_sift_entry_points_are_declared_and_exported():
    from comet_amd import _lib
    src = open(os.path.join(ROOT, "include", "comet_hip.h")).read()
    declared = set(re.findall(r"^\s*int\s+(comet_\w+)\(", src, re.M))
    lib = _lib.load()
    for n in NAMES:
        assert n in declared and n in _lib.SIGNATURES and hasattr(lib, n), n


def test_gauss_blur_rejects_a_radius_over_the_tile_limit():
    from comet_amd import _lib
    lib = _lib.load()
    keep, p = _ptr()
    EINVAL = -1
    # sigma 2.7: r = (round(22.6) | 1) / 2 = 11 > 10
    assert lib.comet_gauss_blur(p, p + 2048, 1, 8, 8, 2.7, None) == EINVAL
    assert b"radius" in lib.comet_last_error()
    assert lib.comet_gauss_blur(p, p + 2048, 1, 8, 8, 0.0, None) == EINVAL
    assert lib.comet_gauss_blur(p, p + 2048, 1, 8, 8, float("nan"), None) == EINVAL


def test_sift_entry_points_reject_zero_sized_images():
    from comet_amd import _lib
    lib = _lib.load()
    keep, p = _ptr()
    EINVAL = -1
    for H, W in ((0, 8), (8, 0)):
        assert lib.comet_gauss_blur(p, p + 2048, 1, H, W, 1.0, None) == EINVAL
        assert lib.comet_sift_base(p, p + 2048, 1, H, W, None) == EINVAL
        assert lib.comet_downsample2(p, p + 2048, 1, H, W, None) == EINVAL
        assert lib.comet_sift_detect(p, 1, 4, H, W, 0, 0.0066667, 10.0, 1.6, p + 1024, 16, p + 2048, p + 2052,
                                     None) == EINVAL
        assert b"bad args" in lib.comet_last_error()
    assert lib.comet_gauss_blur(p, p + 2048, 0, 8, 8, 1.0, None) == EINVAL
