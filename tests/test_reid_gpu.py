"""comet_landmark_reid on the GPU against the float64 restatement tests/reid_numpy.py (DESIGN.md "Landmark
archive"): a constructed case in which every state, every reason a dying row is not retirable, both tie rules,
a pad, NaN / Inf pixels and a retirement on a just-consumed entry occur, at the smallest shapes that cross a
256-thread chunk, a non-multiple of 64, C below the deaths, C = 1 and the LDS maximum, in both rotation
conventions. Every input set is first checked on the CPU: each comparison that decides an outcome sits at
least 1e-6 (relative) from its threshold, but for the constructed exact ties."""
import ctypes

import numpy as np
import pytest
import torch

import landmark_numpy as lmn
import reid_numpy as rn

pytestmark = pytest.mark.gpu

from reid_cases import INTR, MIN_COS, MIN_OBS, MIN_PIVOT, REID_PX, SHAPES, BORN, _case, _check_margins, _pose, _reference, _sphere

def _run_gpu(c, C, inverse, hops=None):
    """The launch on copies of the state -> (ReidOut, acc, acc_id, state) as numpy."""
    from comet_amd import ops
    dev = "cuda"
    hops = list(range(len(c["sidx"]))) if hops is None else hops
    g = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    acc, acc_id = g(c["acc"]), g(c["acc_id"])
    st = {k: g(v) for k, v in c["state"].items()}
    n = len(hops)
    sidx = np.ascontiguousarray(c["sidx"][hops])
    intr = np.ascontiguousarray(c["intr"][hops])
    ws = torch.full((n, c["tracks"].shape[2], 12), float("nan"), dtype=torch.float64, device=dev)
    out = ops.landmark_reid(g(c["tracks"][hops]), g(c["R"][hops]), g(c["T"][hops]), g(c["ids"][hops]), g(c["src"][hops]),
                            g(sidx), (ctypes.c_int32 * n)(*sidx.tolist()), g(intr),
                            (ctypes.c_double * (4 * n))(*intr.reshape(-1).tolist()), acc, acc_id, st["alias"], st["arch"],
                            st["arch_id"], st["arch_cursor"], ws, REID_PX, MIN_COS, MIN_OBS, inverse, MIN_PIVOT)
    torch.cuda.synchronize()
    return ({k: getattr(out, k).cpu().numpy() for k in out._fields}, acc.cpu().numpy(), acc_id.cpu().numpy(),
            {k: v.cpu().numpy() for k, v in st.items()})


def _rel(a, b):
    with np.errstate(all="ignore"):
        d = np.abs(a - b) / np.maximum(np.abs(b), 1e-300)
    d[(a == b) | (np.isnan(a) & np.isnan(b))] = 0.0
    return float(d.max()) if d.size else 0.0


def _compare(got, want):
    gout, gacc, gacc_id, gst = got
    wout, wacc, wacc_id, wst = want
    for k in ("src_lm", "lm_id", "reid_state", "stats"):
        assert np.array_equal(gout[k], wout[k]), k
    assert np.array_equal(gacc_id, wacc_id)
    for k in ("arch_id", "arch_cursor", "alias"):
        assert np.array_equal(gst[k], wst[k]), k
    figures = dict(acc=_rel(gacc, wacc), arch=_rel(gst["arch"][:, :12], wst["arch"][:, :12]),
                   X=_rel(gst["arch"][:, 12:18], wst["arch"][:, 12:18]), dist=_rel(gout["reid_dist"], wout["reid_dist"]))
    print("max relative difference: " + ", ".join(f"{k} {v:.3e}" for k, v in figures.items()))
    assert max(figures["acc"], figures["arch"], figures["X"]) <= 1e-10, figures
    assert figures["dist"] <= 1e-6, figures
    assert (gst["arch"][:, 18:] == 0).all()
    return figures


@pytest.mark.parametrize("shape,inverse", [(s, i) for s in SHAPES[:4] for i in (0, 1)] + [(SHAPES[4], 0)])
def test_constructed_case_matches_the_restatement(shape, inverse):
    n, N, C, T = shape
    c = _case(n, N, C, T, inverse)
    want = _reference(c, C, inverse)
    out = want[0]
    ties = set() if N == 1 else {(h, j) for h in range(n) for j in (14, 15)}
    _check_margins(c, out, ties)
    for h, mk in enumerate(c["marks"]):
        s, state, stats = mk["stream"], out["reid_state"][h], out["stats"][h]
        j = mk["matched_own_retires"]
        assert state[j] == rn.MATCHED and out["src_lm"][h, j] == j and want[2][s * N + j] == c["ids"][h, j]
        # its old row was retired in the same launch, onto the entry it consumed
        e = s * C + mk["consumed_entry"]
        if stats[0] <= C:  # (else the ring came round to it again); slot 3's row is archived under its alias
            assert want[3]["arch_id"][e] == (5 if N == 1 else 6), "the first retirement reuses the consumed entry"
        if N == 1:
            assert out["lm_id"][h, 0] == 77 and tuple(stats) == (1, 1, 1, 0)
            continue
        assert np.array_equal(state[:18], [0, 0, 0, 0, 0, 0, 0, 0, 1, 2, 2, 2, 1, 3, 1, 3, 2, 2])
        assert set(np.unique(state)) == {0, 1, 2, 3}
        assert np.array_equal(out["lm_id"][h, :3], [-1, 4, 12]) and out["lm_id"][h, 8] == 70 and out["lm_id"][h, 14] == 72
        assert np.isposinf(out["reid_dist"][h][state != 1]).all() and (out["reid_dist"][h][state == 1] < REID_PX).all()
        assert stats[0] == 2 + sum(1 for j in range(18, N) if j % 4) and stats[1] == 3
        assert out["cand"][h, mk["etb"]] and not out["cand"][h, mk["e16"]] and out["cos"][h, mk["e16"]] < 0
        # the four dying rows that are not retirable, one for each reason
        piv, thr = out["pivots"][h], MIN_PIVOT * out["diag"][h]
        assert (piv[4] <= thr[4]).any() and (piv[[5, 6, 7]] > thr[[5, 6, 7], None])[[1, 2]].all()
        assert c["acc"][s * N + 5, 10] == 2 and np.isnan(piv[5]).all(), "too few observations: never solved for the record"
        assert np.isnan(lmn.solve(list(c["acc"][s * N + 7]), MIN_PIVOT)[0]).any()
        if stats[0] > C:
            assert stats[3] >= stats[0] - C
    if (n, N, C) == (1, 64, 32):
        assert out["stats"][0, 0] > C and out["stats"][0, 3] > 0, "more deaths than entries: the ring wraps and overwrites"
    got = _run_gpu(c, C, inverse)
    _compare(got, want)
    if N > 1:
        assert np.isnan(want[3]["arch"]).sum() == 0 and np.isnan(got[3]["arch"]).sum() == 0


def test_three_hops_in_one_launch_equal_three_single_launches():
    n, N, C, T = SHAPES[1]
    c = _case(n, N, C, T, 0)
    all_out, all_acc, all_acc_id, all_st = _run_gpu(c, C, 0)
    for h in range(n):
        out, acc, acc_id, st = _run_gpu(c, C, 0, hops=[h])
        s = int(c["sidx"][h])
        for k in out:
            assert out[k][0].tobytes() == all_out[k][h].tobytes(), k
        rows, ents = slice(s * N, (s + 1) * N), slice(s * C, (s + 1) * C)
        assert acc[rows].tobytes() == all_acc[rows].tobytes() and acc_id[rows].tobytes() == all_acc_id[rows].tobytes()
        assert st["alias"][rows].tobytes() == all_st["alias"][rows].tobytes()
        assert st["arch"][ents].tobytes() == all_st["arch"][ents].tobytes()
        assert st["arch_id"][ents].tobytes() == all_st["arch_id"][ents].tobytes()
        assert st["arch_cursor"][s] == all_st["arch_cursor"][s]
        other = np.ones(len(acc_id), bool)
        other[rows] = False
        assert acc[other].tobytes() == c["acc"][other].tobytes(), "a hop writes the rows of its stream only"


@pytest.mark.parametrize("inverse", [0, 1])
def test_a_restored_row_is_added_to_by_the_landmark_update(inverse):
    """A track dies (its slot pads), its landmark is archived, a new track is born on its projection: with
    src_lm, comet_landmark_update adds the hop's frame to the restored row; with src it starts over."""
    from comet_amd.stream import LandmarkMap
    N, T, C = 64, 4, 8
    X = _sphere(1, 3) * 0.5
    poses = [_pose(f, 0) for f in range(12)]
    px = np.stack([lmn.project(X, q, t, INTR, inverse)[0][0] for q, t in poses]).astype(np.float32)
    lm = LandmarkMap(T, 1, 1, N, [INTR], inverse_rotation=inverse, archive=C, reid_px=REID_PX)
    acc, acc_id = lmn.new_state(1, N)
    st = rn.new_state(1, N, C)
    j = 5
    plan = [(7, BORN), (7, j), (7, j), (7, j), (-1, rn.INT_MIN), (-1, rn.INT_MIN), (9, BORN), (9, j)]
    for k, (ident, source) in enumerate(plan):
        tracks = np.full((1, T, N, 2), -500.0, np.float32)
        tracks[0, :, j] = px[k:k + T]
        R = np.stack([poses[k + i][0] for i in range(T)])[None].astype(np.float32)
        Tx = np.stack([poses[k + i][1] for i in range(T)])[None]
        ids, src = np.full((1, N), -1, np.int32), np.full((1, N), rn.INT_MIN, np.int32)
        ids[0, j], src[0, j] = ident, source
        want = rn.reid(tracks, R, Tx, ids, src, [0], np.array([INTR]), acc, acc_id, st, C, REID_PX, MIN_COS, MIN_OBS,
                       inverse, MIN_PIVOT)
        wlo = lmn.update(tracks, R, Tx, ids, want["src_lm"], [0], np.array([INTR]), acc, acc_id, 1, inverse_rotation=inverse)
        g = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
        ro = lm.reidentify([0], g(tracks), g(R), g(Tx), g(ids), g(src))
        lo = lm.update([0], g(tracks), g(R), g(Tx), g(ids), ro.src_lm)
        assert np.array_equal(ro.reid_state.cpu().numpy(), want["reid_state"])
        assert np.array_equal(ro.lm_id.cpu().numpy(), want["lm_id"]) and np.array_equal(ro.stats.cpu().numpy(), want["stats"])
        assert np.array_equal(lo.n_obs.cpu().numpy(), wlo["n_obs"]) and np.array_equal(lo.state.cpu().numpy(), wlo["state"])
        assert _rel(lm.acc.cpu().numpy(), acc) <= 1e-10
        if k == 4:
            assert want["stats"][0, 0] == 1, "the dead track's row is archived"
        if k == 6:
            assert want["reid_state"][0, j] == rn.MATCHED and want["lm_id"][0, j] == 7
            assert wlo["n_obs"][0, j] == 5 and wlo["state"][0, j] == lmn.VALID, "4 archived frames + this hop's, valid at birth"
            plain = lmn.update(tracks, R, Tx, ids, src, [0], np.array([INTR]), acc.copy(), acc_id.copy(), 1,
                               inverse_rotation=inverse)
            assert plain["n_obs"][0, j] == 1
    ids_s, X_s, n_s = lm.snapshot(0)
    assert ids_s.tolist() == [7] and n_s.tolist() == [6], "the snapshot names the landmark, not the carry's track"
    assert np.abs(X_s.cpu().numpy()[0] - X[0]).max() <= 1e-4  # (f32 pixels: ~1e-5 px)
    lm.reset(0)
    assert lm.archive_snapshot(0)[0].numel() == 0 and (lm.alias == -1).all() and (lm.arch_cursor == 0).all()
