"""The yardstick of the SIFT tests (tests/sift_numpy.py) checked on its own, without a GPU: an
analytic blob check, and the float32-vs-float64 noise floor that the GPU tests' tolerances come from."""
import math

import numpy as np
import pytest

import sift_numpy as S


@pytest.mark.parametrize("s", [2.0, 3.0, 4.5])
def test_restatement_finds_an_isotropic_blob(s):
    """A single Gaussian blob of std s centred off-grid: the strongest keypoint lies within 0.5 px of
    the centre and its size / 2 within a factor sqrt(2) of s (about two layer steps: a sanity bound)."""
    cy, cx = 31.3, 33.6
    kps = S.detect(S.blob_image(64, 64, cy, cx, s))
    assert kps
    k = kps[0]
    assert math.hypot(k["x"] - cx, k["y"] - cy) <= 0.5, (k["x"], k["y"])
    assert s / math.sqrt(2) <= k["size"] / 2 <= s * math.sqrt(2), k["size"]


def test_float32_agrees_with_float64_off_the_margins():
    """On each test image: at least 20 float64 keypoints, at most 10 % of them marginal, and the
    float32 run holds every non-marginal one (same octave, layer and orientation count) and nothing
    that matches no float64 keypoint. The floors printed here are the ones DESIGN.md §11 records."""
    ref = S.reference()
    print("float32-vs-float64 floors:", ref["floor"])
    for hw in S.SHAPES:
        for k64, k32 in zip(ref["kp64"][hw], ref["kp32"][hw]):
            marg = [S.is_marginal(k) for k in k64]
            print(hw, "keypoints", len(k64), "marginal", sum(marg))
            assert len(k64) >= 20
            assert sum(marg) <= 0.1 * len(k64)
            for k, j, mg in zip(k64, S.match(k64, k32), marg):
                if not mg:
                    assert j is not None, k
                    assert k32[j]["nori"] == k["nori"], (k, k32[j])
            assert all(j is not None for j in S.match(k32, k64))
    f = ref["floor"]
    assert 0 < f["image"] < 1e-3 and 0 < f["pos"] < 1e-2 and 0 < f["size"] < 1e-2 and 0 < f["response"] < 1e-5


def test_selection_rules_on_a_hand_made_list():
    """keep-best-n over the orientation-expanded list keeps every tie with the last kept response;
    of two candidates on one pixel the better stays; the max filter drops a weaker neighbour; top-k."""
    #        0     1     2     3     4     5     6
    x = [10.6, 10.9, 20.5, 30.5, 31.5, 40.5, 50.5]
    y = [10.6, 10.7, 20.5, 30.5, 30.5, 40.5, 50.5]
    resp = [0.9, 0.8, 0.7, 0.6, 0.5, 0.5, 0.4]
    nori = [1, 1, 2, 1, 1, 1, 1]
    # n = 6 expanded entries: 0, 1, 2, 2, 3, 4 -> last response 0.5, its tie (5) stays, 6 goes;
    # 1 shares pixel (10, 10) with 0 and goes; then the top 5 of [0, 2, 3, 4, 5]
    assert list(S.select(x, y, resp, nori, 64, 64, 6)) == [0, 2, 3, 4, 5]
    # n = 4: 0, 1, 2, 2 -> last response 0.7; 1 goes with its pixel
    assert list(S.select(x, y, resp, nori, 64, 64, 4)) == [0, 2]
    # radius 1: 4 (0.5) sits next to 3 (0.6) and goes
    assert list(S.select(x, y, resp, nori, 64, 64, 6, nms_radius=1)) == [0, 2, 3, 5]
    # three ties at the cut all pass keep-best-n; the final top-k takes the first of the sorted list
    assert list(S.select([5.5, 15.5, 25.5, 35.5], [5.5] * 4, [0.9, 0.5, 0.5, 0.5], [1] * 4, 64, 64, 2)) == [0, 1]
    assert list(S.select([5.5], [5.5], [0.9], [0], 64, 64, 2)) == []
