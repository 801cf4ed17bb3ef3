"""The SIFT detector of comet_amd.keypoints on the GPU against the float64 restatement of its rules
(tests/sift_numpy.py): the scale-space kernels image by image, the detector keypoint by keypoint,
extract() end to end, and the way through keypoint_tracks and the loop's config key.

Tolerances are 4x the float32-vs-float64 floors of the restatement itself (tests/test_sift_cpu.py
asserts the conditions they rest on; DESIGN.md §11 records the values): the kernels sum in another
order than numpy's float32 run and contract multiply-adds, which is worth a small factor and no more."""
import numpy as np
import pytest
import torch

import sift_numpy as S

pytestmark = pytest.mark.gpu
MARGIN = 4.0


@pytest.fixture(scope="module")
def ref():
    return S.reference()


def _call(name, *args):
    from comet_amd import _lib as L
    from comet_amd import ops
    L.check(getattr(L.load(), name)(*args, ops.stream()), name)


def _blur(x, sigma):
    y = torch.empty_like(x)
    B, H, W = x.shape
    _call("comet_gauss_blur", x.data_ptr(), y.data_ptr(), B, H, W, float(sigma))
    return y


def test_base_image_matches_the_restatement(ref):
    tol = MARGIN * ref["floor"]["image"]
    for hw, imgs in S.images().items():
        g = torch.from_numpy(imgs).cuda()
        B, H, W = g.shape
        base = torch.empty(B, 2 * H, 2 * W, device="cuda")
        _call("comet_sift_base", g.data_ptr(), base.data_ptr(), B, H, W)
        want = np.stack([ref["pyr64"][hw][i][0][0] for i in range(B)])
        err = np.abs(base.cpu().numpy().astype(np.float64) - want).max()
        print(hw, "base image max err", err, "tol", tol)
        assert err <= tol


@pytest.mark.parametrize("octave", [0, 3, 4])
def test_gauss_blur_matches_the_restatement(ref, octave):
    """The six blurs of one octave of the 97 x 83 images, each from the float64 layer below it:
    octave 0 (194 x 166: several tiles, neither side a multiple of the tile), octave 3 (24 x 20: the
    radius reaches the image size) and octave 4 (12 x 10: the border reflects more than once)."""
    tol = MARGIN * ref["floor"]["image"]
    hw = S.SHAPES[1]
    G = np.stack([ref["pyr64"][hw][i][octave] for i in range(2)])  # [B, 7, h, w]
    for i, sigma in enumerate(S.layer_sigmas(4), start=1):
        got = _blur(torch.from_numpy(G[:, i - 1].astype(np.float32)).cuda().contiguous(), sigma)
        err = np.abs(got.cpu().numpy().astype(np.float64) - G[:, i]).max()
        print("octave", octave, "layer", i, "sigma %.4f" % sigma, "max err", err, "tol", tol)
        assert err <= tol


def test_downsample2_takes_every_second_pixel():
    g = torch.Generator().manual_seed(3)
    for H, W in ((97, 83), (12, 10), (2, 3)):
        x = torch.randn(2, H, W, generator=g).cuda()
        y = torch.empty(2, H // 2, W // 2, device="cuda")
        _call("comet_downsample2", x.data_ptr(), y.data_ptr(), 2, H, W)
        assert torch.equal(y, x[:, 0:2 * (H // 2):2, 0:2 * (W // 2):2])


def _as_dicts(c):
    keys = ("x", "y", "size", "response", "nori", "octave", "layer")
    return [dict(zip(keys, (float(v) for v in row))) for row in c.cpu().numpy()]


@pytest.mark.parametrize("hw", S.SHAPES)
def test_detector_matches_the_restatement(ref, hw):
    """The candidate list before any cut holds every non-marginal float64 keypoint (same octave,
    layer and orientation count; position, size and response within 4x the floors) and nothing that
    matches no float64 keypoint."""
    from comet_amd.keypoints import SIFT
    f = ref["floor"]
    lists = SIFT().detect(torch.from_numpy(S.images()[hw]).cuda())
    for k64, c in zip(ref["kp64"][hw], lists):
        got = _as_dicts(c)
        worst = {"pos": 0.0, "size": 0.0, "response": 0.0}
        fails = []
        for k, j in zip(k64, S.match(k64, got)):
            if S.is_marginal(k):
                continue
            if j is None:
                fails.append(("missing", k))
                continue
            q = got[j]
            d = {"pos": max(abs(q["x"] - k["x"]), abs(q["y"] - k["y"])), "size": abs(q["size"] - k["size"]),
                 "response": abs(q["response"] - k["response"])}
            for n in worst:
                worst[n] = max(worst[n], d[n])
            if int(q["nori"]) != k["nori"] or any(d[n] > MARGIN * f[n] for n in d):
                fails.append(("differs", k, q))
        extra = [q for q, j in zip(got, S.match(got, k64)) if j is None]
        print(hw, "float64", len(k64), "gpu", len(got), "worst", worst, "floors", f)
        assert not fails, fails
        assert not extra, extra


def _rgb(gray_u8):
    """uint8 [B, H, W] -> float [B, 3, H, W] in [0, 1]"""
    return (torch.from_numpy(gray_u8).float() / 255.0)[:, None].expand(-1, 3, -1, -1).contiguous().cuda()


def test_selection_matches_the_restatement():
    """keep-best-n with its tie rule, the same-pixel rule, the max filter and the top-k on a
    hand-made list with two candidates on one pixel and two equal responses at the cut."""
    from comet_amd.keypoints import SIFT
    x = [10.6, 10.9, 20.5, 30.5, 31.5, 40.5, 50.5]
    y = [10.6, 10.7, 20.5, 30.5, 30.5, 40.5, 50.5]
    resp = [0.9, 0.8, 0.7, 0.6, 0.5, 0.5, 0.4]
    nori = [1, 1, 2, 1, 1, 1, 1]
    cases = [(x, y, resp, nori)]
    cases.append(([5.5, 15.5, 25.5, 35.5], [5.5] * 4, [0.9, 0.5, 0.5, 0.5], [1] * 4))
    cases.append(([5.5], [5.5], [0.9], [0]))
    for cx, cy, cr, cn in cases:
        z = [0.0] * len(cx)
        cand = torch.tensor([cx, cy, z, cr, cn, z, z], dtype=torch.float32).t().contiguous().cuda()
        for mk in (2, 4, 6, None):
            for r in (0, 1):
                got = SIFT(max_num_keypoints=mk, nms_radius=r).select(cand, 64, 64).cpu().tolist()
                want = [int(v) for v in S.select(cx, cy, cr, cn, 64, 64, mk, nms_radius=r)]
                assert got == want, (mk, r, got, want)


def test_extract_is_deterministic_batched_and_handles_an_empty_image():
    from comet_amd.keypoints import SIFT
    sift = SIFT(resize=None)
    img = _rgb(S.images()[(64, 64)])
    a, b = sift.extract(img), sift.extract(img)
    assert set(a) >= {"keypoints", "keypoint_scores", "scales"}
    for k in a:
        assert torch.equal(a[k], b[k]), k
    n = a["num_keypoints"].tolist()
    assert a["keypoints"].shape == (2, max(n), 2) and min(n) >= 20
    for i in range(2):
        one = sift.extract(img[i])
        assert one["keypoints"].shape == (1, n[i], 2)
        for k in ("keypoints", "keypoint_scores", "scales"):
            assert torch.equal(one[k][0], a[k][i, :n[i]]), (i, k)
        sc = one["keypoint_scores"][0]
        assert bool((sc[:-1] >= sc[1:]).all())
    flat = sift.extract(torch.full((3, 64, 64), 0.5, device="cuda"))
    assert flat["keypoints"].shape == (1, 0, 2) and flat["keypoint_scores"].shape == (1, 0)
    mixed = sift.extract(torch.cat([img[:1], torch.full((1, 3, 64, 64), 0.5, device="cuda")]))
    assert mixed["num_keypoints"].tolist() == [n[0], 0]


def test_candidate_overflow_raises():
    from comet_amd._lib import CometHipError
    from comet_amd.keypoints import SIFT
    with pytest.raises(CometHipError, match="candidate_capacity"):
        SIFT(candidate_capacity=4).detect(torch.from_numpy(S.images()[(64, 64)]).cuda())


def test_keypoint_tracks_takes_a_sift(ref):
    from comet_amd.keypoints import SIFT, SuperPoint, keypoint_tracks
    torch.manual_seed(0)
    sp = SuperPoint(max_num_keypoints=64, detection_threshold=0.005, resize=None).cuda()
    sift = SIFT(max_num_keypoints=64, resize=None)
    imgs = _rgb(S.images()[(64, 64)])[:, None].expand(-1, 3, -1, -1, -1).contiguous()  # [B, T, 3, H, W]
    mask = torch.zeros(2, 64, 64, dtype=torch.bool, device="cuda")
    mask[:, 8:56, 8:56] = True
    tracks, vis = keypoint_tracks(sp, imgs, mask, track_num=200, sift=sift, min_required=200)
    assert tracks.shape == (2, 3, 200, 2) and vis.shape == (2, 3, 200) and bool(vis.all())
    for i in range(2):
        kp = sift.extract(imgs[i, 0])["keypoints"][0]
        xs, ys = kp[:, 0].round().clamp(0, 63).long(), kp[:, 1].round().clamp(0, 63).long()
        inside = kp[mask[i][ys, xs]]
        assert inside.shape[0] >= 10
        d = (tracks[i, 0][None] - inside[:, None]).abs().amax(-1)  # [n_inside, 200]
        assert bool((d.amin(1) == 0).all())


def test_loop_builds_a_sift_only_on_request():
    from comet_amd import loop
    from comet_amd.keypoints import SIFT
    assert loop._sift_init({"train": {"track_num": 128}}, "cuda") is None
    assert loop._sift_init({"train": {"track_num": 128, "track_by_sift": False}}, "cuda") is None
    s = loop._sift_init({"train": {"track_num": 128, "track_by_sift": True}}, "cuda")
    assert isinstance(s, SIFT) and s.conf["max_num_keypoints"] == 128
