"""CPU-side checks of the tracker entry points of libcomet_hip.so: bad arguments are rejected on
the host, with a message naming the constraint, before anything is launched (the pointers are
aligned host addresses that are never read)."""
import ctypes

import pytest

EINVAL = -1


def _lib():
    from comet_amd import _lib as L
    return L, L.load()


def _ptr():
    buf = ctypes.create_string_buffer(1 << 12)
    return buf, ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256


def test_patch_gather_rejects_a_frame_narrower_than_high():
    """Both patch origins are clamped with H - P (refine_track.py:104 uses H for x as well), so with
    W < H the clamped x origin can pass W - P and the patch would be read past the row or frame."""
    L, lib = _lib()
    keep, p = _ptr()
    for H, W in ((40, 32), (40, 39), (8, 7)):
        rc = lib.comet_patch_gather(L.F32, p, p, p, p, p, 1, 2, 4, H, W, 3, 3, None)
        assert rc == EINVAL and b"W >= H" in lib.comet_last_error(), (H, W)
    for H, W in ((5, 40), (40, 5), (6, 6)):  # a frame smaller than the 7 x 7 patch, either way round
        rc = lib.comet_patch_gather(L.F32, p, p, p, p, p, 1, 2, 4, H, W, 3, 3, None)
        assert rc == EINVAL and b"smaller than a patch" in lib.comet_last_error(), (H, W)


@pytest.mark.parametrize("cpad", [0, 2, 9])
def test_patch_gather_and_images_nhwc_reject_a_channel_pad_outside_3_to_8(cpad):
    L, lib = _lib()
    keep, p = _ptr()
    rc = lib.comet_patch_gather(L.BF16, p, p, p, p, p, 1, 2, 4, 40, 40, 3, cpad, None)
    assert rc == EINVAL and b"cpad must be in [3, 8]" in lib.comet_last_error()
    rc = lib.comet_images_nhwc(L.BF16, p, p, 2, 6, 10, 3, 5, cpad, None)
    assert rc == EINVAL and b"cpad must be in [3, 8]" in lib.comet_last_error()


@pytest.mark.parametrize("sradius,P", [(0, 9), (3, 9), (-1, 9), (2, 4)])
def test_track_score_rejects_a_search_radius_other_than_1_or_2(sradius, P):
    L, lib = _lib()
    keep, p = _ptr()
    rc = lib.comet_track_score(L.F32, p, p, p, p, p, 2, 4, 5, P, 32, sradius, None)
    assert rc == EINVAL and b"sradius must be 1 or 2" in lib.comet_last_error()


def test_tracker_tokens_rejects_rows_narrower_than_their_content():
    L, lib = _lib()
    keep, p = _ptr()
    # row pitch below the token width
    rc = lib.comet_tracker_tokens(L.BF16, p, p, 32, p, 147, 147, p, 216, p, 200, 16, 4, None)
    assert rc == EINVAL and b"bad args" in lib.comet_last_error()
    # token width below flow embedding + flow + corr + feats (2*128 + 2 + 324 = 582 > 580)
    rc = lib.comet_tracker_tokens(L.F32, p, p, 128, p, 324, 324, p, 580, p, 580, 30, 3, None)
    assert rc == EINVAL and b"bad args" in lib.comet_last_error()


@pytest.mark.parametrize("C", [64, 12, 256])
def test_corr_sample_rejects_channel_counts_other_than_32_and_128(C):
    L, lib = _lib()
    keep, p = _ptr()
    ptrs = (ctypes.c_void_p * 3)(p, p, p)
    hw = (ctypes.c_int * 3)(8, 4, 2)
    rc = lib.comet_corr_sample(L.F32, L.F32, ptrs, hw, hw, 3, 3, C, p, p, p, 147, 0, 1, 4, 2, None)
    assert rc == EINVAL and b"C must be 128 (coarse) or 32 (fine)" in lib.comet_last_error()
