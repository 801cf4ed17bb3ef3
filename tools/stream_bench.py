"""Online inference: time per hop of comet_amd.stream.PoseStream against the closed-window call.

    python tools/stream_bench.py [--frames 16 --image 512 --tracks 512 --hops 32 --warmup 4]
    python tools/stream_bench.py --streams 1,2,4,8      (the stream pool, see below)

Synthetic frames of the SURVEY 8(d) recipe (N(0,1) frames, U[0, S-1] query points), random-init
weights, bf16, stride 1. After the warm-up hops, `--hops` hops each of
  (a) stream   one push of the newest frame: its per-frame stages, the ring store, the gather, the
               cross-frame part of the model;
  (b) closed   the same windows through model(window, training=False, tracks=...), what a caller
               without the stream runs per hop;
  (c) gather   the comet_ring_gather launch alone (with the bytes it moves: achieved bandwidth).
Each hop is timed with device events; the figures are medians. (a) and (b) alternate hop by hop, so
both see the same machine state. One JSON line. Needs a GPU (no fallback).

--streams S[,S...]: comet_amd.stream.StreamPool against separate streams instead, one JSON line per
S. Every stream has its own frames; all are in phase, so every timed push completes S hops. Per push
  (a) pool      one StreamPool.push of S frames: the per-frame stages at batch S, one
                comet_ring_scatter, one comet_ring_gather, the cross-frame part at B = S;
  (b) separate  S independent PoseStream objects pushed one after another with the same frames (what
                a caller without the pool runs);
  (c) scatter   the comet_ring_scatter launch of a push alone, into a scratch ring (with the bytes it
                moves: achieved bandwidth).
(a) and (b) alternate push by push in one process; device events, medians and minima.

--fuse: pose fusion (comet_pose_fuse, DESIGN.md "Pose fusion") against the chained decode it replaces.
Two anchored streams (with --streams: two anchored pools of S streams) take the same frames,
  (a) fuse on   one comet_pose_fuse launch per push for the absolute poses;
  (b) fuse off  two comet_pose_decode launches and the torch arithmetic of _decode_chained per hop;
  (c) kernel    the comet_pose_fuse launch of a push alone, on a scratch PoseFuser.
(a) and (b) alternate push by push in one process; device events, medians and minima.

--carry [--detect-every K] [--min-score V]: track carry (comet_track_carry, DESIGN.md "Track carry")
against the detector on every hop. Needs the SuperPoint weights of cfg (as loop.stream_eval does).
Three PoseStream objects take the same frames, alternating hop by hop in one process:
  (a) query_fn  query_fn = keypoint_query(sp): SuperPoint + filter_and_pad on every hop (the path before);
  (b) carry 1   carry=True, detect_every=1: SuperPoint on every hop, no filter_and_pad;
  (c) carry K   carry=True, detect_every=K (default 4);
  (d) kernel    the comet_track_carry launch of (b)'s hop alone (20 back-to-back launches / 20).
Also per timed hop of (b) and (c): survivors, born, padded and the mean age, and the largest
pred_pose_enc difference between (a) and (b) on the same windows (a difference between two query
sets, not an error against ground truth). Random-init weights and N(0,1) frames: the tracks say little
about real imagery.

--carry --warm [--warm-iters K[,K...]] [--warm-mode hold|velocity]: the warm start of the coarse tracker
(comet_track_warm, DESIGN.md "Warm start") joins the alternation: one more PoseStream per K with
carry=True, detect_every=1, warm=True, warm_iters=K (default: cfg.track_trainit), to be read against
(b) carry 1. Also the comet_track_warm launch of a hop alone (20 back-to-back launches / 20), per timed
hop the slots that started warm, and the largest pred_tracks / pred_pose_enc difference between each
warm stream and (b) on the same frames: a difference between two tracker runs under random-init
weights, which converge to nothing meaningful, so it is not an accuracy figure.

--fuse --carry --landmarks: the landmark map (comet_landmark_update, DESIGN.md "Landmarks"): two
PoseStream(fuse=True, carry=True) objects, landmarks on and off, alternate push by push in one process;
ms per push of each, the comet_landmark_update launch of a hop alone (20 back-to-back launches / 20), the
valid landmarks per hop and whether pred_pose_enc stayed identical. A report, not a pass criterion.
--fuse --carry --landmarks --reid: the landmark archive (comet_landmark_reid, DESIGN.md "Landmark archive"): two
PoseStream(fuse=True, carry=True, landmarks=True) objects, lm_archive on and off, alternate push by push in
one process; ms per push of each and the comet_landmark_reid launch of a hop alone. A report.
--fuse --carry --landmarks --pnp: the PnP refinement (comet_landmark_pnp, DESIGN.md "PnP refinement"): two
PoseStream(fuse=True, carry=True, landmarks=True) objects, pnp on (report only, pnp_weight 0) and off,
alternate push by push in one process; ms per push of each, the comet_landmark_pnp launch of a hop alone
(20 back-to-back launches / 20), the solved positions per hop and whether pred_pose_enc stayed identical.
A report, not a pass criterion.
--fuse --motion: the motion estimate (comet_motion_fit, DESIGN.md "Motion estimate"): two PoseStream(fuse=True)
objects with fixed query points, motion on and off, alternate push by push in one process; ms per push of
each, the comet_motion_fit launch of a hop alone (20 back-to-back launches / 20), the states seen and whether
pred_pose_enc and the fused poses stayed identical. A report, not a pass criterion."""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

import torch

GATHER_REPS = 20
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "comet-pose-estimation_amd"))


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def pool_bench(model, n_streams, args, dev):
    from comet_amd import ops
    from comet_amd.stream import PoseStream, StreamPool
    T, S, N = args.frames, args.image, args.tracks
    g = torch.Generator(device=dev).manual_seed(1)
    total = T + args.warmup + args.hops - 1
    frames = torch.randn(total, n_streams, 3, S, S, device=dev, generator=g)  # frames[f]: one push
    q = torch.rand(N, 2, device=dev, generator=g) * (S - 1)
    pool = StreamPool(model, streams=n_streams, window=T, stride=1, precision=torch.bfloat16)
    singles = [PoseStream(model, window=T, stride=1, precision=torch.bfloat16) for _ in range(n_streams)]

    def separate(f):
        return [st.push(frames[f, s], query_points=q) for s, st in enumerate(singles)]

    for f in range(T - 1):
        assert pool.push(frames[f], query_points=q) == [] and not any(separate(f))
    live = [(w, r) for w, r in zip(pool._wins, pool._rings) if r is not None]
    srcs = [w[:n_streams] for w, _ in live]           # k = S rows of each cached kind
    scratch = [torch.empty_like(r) for _, r in live]  # (the pool's own rings are left alone)
    ta, tb, tc, err = [], [], [], 0.0
    for k in range(args.warmup + args.hops):
        f = k + T - 1
        ms_a, res = _timed(lambda: pool.push(frames[f], query_points=q))
        ms_b, ref = _timed(lambda: separate(f))
        assert [s for s, _ in res] == list(range(n_streams)) and all(len(r) == 1 for r in ref)
        slots = [pool.sched.slot(s, f) for s in range(n_streams)]
        table, table_host = pool._table(slots)
        ms_c, _ = _timed(lambda: [ops.ring_scatter(list(zip(srcs, scratch)), table, table_host) for _ in range(GATHER_REPS)])
        if k >= args.warmup:
            ta.append(ms_a)
            tb.append(ms_b)
            tc.append(ms_c / GATHER_REPS)
            for (s, r), one in zip(res, ref):
                assert r.frame_index == one[0].frame_index == k
                err = max(err, float((r.pred_pose_enc - one[0].pred_pose_enc).abs().max()))
    nbytes = 2 * n_streams * sum(r[0].numel() * r.element_size() for r in scratch)
    a, b, c = statistics.median(ta), statistics.median(tb), statistics.median(tc)
    print(json.dumps({
        "metric": f"ms per push of {n_streams} streams (each push completes {n_streams} hops), online COMET inference, "
                  f"T={T} {S}^2 N={N}, bf16, stride 1",
        "streams": n_streams, "pool_ms": round(a, 3), "separate_ms": round(b, 3), "separate_over_pool": round(b / a, 3),
        "pool_hops_per_s": round(n_streams * 1e3 / a, 2), "separate_hops_per_s": round(n_streams * 1e3 / b, 2),
        "min_pool_ms": round(min(ta), 3), "min_separate_ms": round(min(tb), 3),
        "scatter_ms": round(c, 4), "min_scatter_ms": round(min(tc), 4), "scatter_bytes_read_plus_written": nbytes,
        "scatter_GBps": round(nbytes / (c * 1e-3) / 1e9, 1),
        "scatter_timing": f"device events around {GATHER_REPS} back-to-back launches / {GATHER_REPS}, median over the pushes",
        "pushes": args.hops, "warmup": args.warmup, "max_abs_pose_enc_diff_pool_vs_separate": err,
        "data": "synthetic (N(0,1) frames, U[0,S-1] query points); random-init weights"}), flush=True)


def fuse_bench(model, n_streams, args, dev):
    """--fuse: n_streams = 0 times PoseStream, else StreamPool with that many streams."""
    from comet_amd.models.utils import INTRINSICS
    from comet_amd.stream import Hop, PoseFuser, PoseStream, StreamPool
    T, S, N = args.frames, args.image, args.tracks
    k = max(n_streams, 1)
    g = torch.Generator(device=dev).manual_seed(1)
    total = T + args.warmup + args.hops - 1
    frames = torch.randn(total, k, 3, S, S, device=dev, generator=g)
    q = torch.rand(N, 2, device=dev, generator=g) * (S - 1)
    R0 = torch.tensor([0.8, 0.2, -0.4, 0.4], device=dev)
    anchor = (R0 / R0.norm(), torch.tensor([331.25, 247.5, 11.375], device=dev), 268.44, 0.5, "AMD")
    if n_streams == 0:
        objs = {f: PoseStream(model, window=T, stride=1, anchor=anchor, precision=torch.bfloat16, fuse=f)
                for f in (True, False)}
        push = lambda f, i: objs[f].push(frames[i, 0], query_points=q)
    else:
        objs = {f: StreamPool(model, streams=k, window=T, stride=1, anchors=[anchor] * k, precision=torch.bfloat16, fuse=f)
                for f in (True, False)}
        push = lambda f, i: [r for _, r in objs[f].push(frames[i], query_points=q)]
    for i in range(T - 1):
        assert push(True, i) == [] and push(False, i) == []
    scratch = PoseFuser(T, 1, T, k, [(anchor[0], anchor[1])] * k, 0.5, INTRINSICS["AMD"], dev)
    ta, tb, tc, err = [], [], [], 0.0
    for j in range(args.warmup + args.hops):
        i = j + T - 1
        order = (True, False) if j % 2 == 0 else (False, True)  # (neither path always runs first)
        ms, res = {}, {}
        for f in order:
            ms[f], res[f] = _timed(lambda: push(f, i))
        assert len(res[True]) == len(res[False]) == k
        enc = torch.stack([r.pred_pose_enc for r in res[True]])
        hops = [(s, Hop(j, j % T)) for s in range(k)]
        ms_c, _ = _timed(lambda: [scratch.fuse(enc, hops) for _ in range(GATHER_REPS)])
        if j >= args.warmup:
            ta.append(ms[True])
            tb.append(ms[False])
            tc.append(ms_c / GATHER_REPS)
            for a, b in zip(res[True], res[False]):
                err = max(err, float((a.pred_pose_enc - b.pred_pose_enc).abs().max()))
    a, b, c = statistics.median(ta), statistics.median(tb), statistics.median(tc)
    print(json.dumps({
        "metric": f"ms per push, pose fusion on against off, {'PoseStream' if n_streams == 0 else f'StreamPool of {k} streams'}, "
                  f"T={T} {S}^2 N={N}, bf16, stride 1",
        "streams": n_streams, "fuse_on_ms": round(a, 3), "fuse_off_ms": round(b, 3), "on_over_off": round(a / b, 4),
        "min_fuse_on_ms": round(min(ta), 3), "min_fuse_off_ms": round(min(tb), 3),
        "pose_fuse_ms": round(c, 4), "min_pose_fuse_ms": round(min(tc), 4), "pose_fuse_hops_per_launch": k,
        "pose_fuse_timing": f"device events around {GATHER_REPS} back-to-back launches / {GATHER_REPS}, median over the pushes",
        "pushes": args.hops, "warmup": args.warmup, "max_abs_pose_enc_diff_on_vs_off": err,
        "data": "synthetic (N(0,1) frames, U[0,S-1] query points); random-init weights"}), flush=True)


def carry_bench(model, args, dev, cfg):
    from comet_amd import loop, ops
    from comet_amd.stream import PoseStream, keypoint_candidates, keypoint_query
    T, S, N = args.frames, args.image, args.tracks
    g = torch.Generator(device=dev).manual_seed(1)
    total = T + args.warmup + args.hops - 1
    frames = torch.randn(total, 3, S, S, device=dev, generator=g)
    sp = loop._keypoint_init(cfg, dev)
    kw = dict(window=T, stride=1, precision=torch.bfloat16)
    ckw = dict(kw, carry=True, carry_tracks=N, carry_cell=args.cell, carry_min_score=args.min_score,
               candidate_fn=keypoint_candidates(sp))
    objs = {"query_fn": PoseStream(model, query_fn=keypoint_query(sp, track_num=N, min_required=N), **kw),
            "carry_1": PoseStream(model, detect_every=1, **ckw),
            "carry_k": PoseStream(model, detect_every=args.detect_every, **ckw)}
    warm_names = {}
    if args.warm:
        for it in ([None] if args.warm_iters is None else [int(v) for v in args.warm_iters.split(",")]):
            name = f"warm_{'cfg' if it is None else it}"
            warm_names[name] = it
            objs[name] = PoseStream(model, detect_every=1, warm=True, warm_mode=args.warm_mode, warm_iters=it, **ckw)
    names = list(objs)
    carried = names[1:3]
    wstats = {k: [] for k in warm_names}
    wdiff = {k: [0.0, 0.0, 0.0] for k in warm_names}  # pred_tracks (all slots, slots with one query), pred_pose_enc
    tw = []
    for o in objs.values():
        assert o.push(frames[:T - 1]) == []
    times = {k: [] for k in names}
    stats = {k: [] for k in carried}
    tk, err = [], 0.0
    for j in range(args.warmup + args.hops):
        i = j + T - 1
        res = {}
        for k in names[j % len(names):] + names[:j % len(names)]:  # (no path always runs first)
            ms, out = _timed(lambda: objs[k].push(frames[i]))
            assert len(out) == 1 and out[0].frame_index == j
            res[k] = (ms, out[0])
        tc = objs["carry_1"]._carry
        cand = objs["carry_1"].candidate_fn(frames[j]).float().contiguous()[None]
        cn = torch.tensor([cand.shape[1]], dtype=torch.int32, device=dev)
        pv = torch.ones(1, dtype=torch.int32, device=dev)
        r = res["carry_1"][1]
        nid = tc.next_id.clone()
        ms_k, _ = _timed(lambda: [ops.track_carry(r.pred_tracks[None], r.pred_score[None].float(), tc.ids, tc.age, nid, pv, 1,
                                                  S, S, args.cell, 0, args.min_score, cand, cn) for _ in range(GATHER_REPS)])
        if args.warm:
            wc = objs[next(iter(warm_names))]._carry
            wq = r.pred_tracks[1].contiguous()[None]
            ms_w, _ = _timed(lambda: [ops.track_warm(r.pred_tracks[None], r.track_src[None], wq, pv, 1, S, S, args.warm_mode,
                                                     *wc.warm_div) for _ in range(GATHER_REPS)])
        if j >= args.warmup:
            for k in names:
                times[k].append(res[k][0])
            tk.append(ms_k / GATHER_REPS)
            if args.warm:
                tw.append(ms_w / GATHER_REPS)
            for k in warm_names:
                a, b = res[k][1], r
                wstats[k].append(int((a.track_warm > 0).sum()))
                same = (a.pred_tracks[0] == b.pred_tracks[0]).all(-1)
                d = (a.pred_tracks - b.pred_tracks).abs()
                wdiff[k][0] = max(wdiff[k][0], float(d.max()))
                if bool(same.any()):
                    wdiff[k][1] = max(wdiff[k][1], float(d[:, same].max()))
                wdiff[k][2] = max(wdiff[k][2], float((a.pred_pose_enc - b.pred_pose_enc).abs().max()))
            err = max(err, float((res["query_fn"][1].pred_pose_enc - res["carry_1"][1].pred_pose_enc).abs().max()))
            for k in carried:
                rr = res[k][1]
                sv, bn, pd = loop._carry_counts(rr)
                live = rr.track_ids >= 0
                stats[k].append((sv, bn, pd, float(rr.track_age[live].float().mean()) if bool(live.any()) else 0.0))
    out = {"metric": f"ms per hop, track carry against a detector + filter_and_pad on every hop, PoseStream, T={T} {S}^2 "
                     f"N={N}, bf16, stride 1", "detect_every": args.detect_every, "carry_min_score": args.min_score,
           "carry_cell": args.cell}
    for k in names:
        out[f"{k}_ms"] = round(statistics.median(times[k]), 3)
        out[f"min_{k}_ms"] = round(min(times[k]), 3)
    out["track_carry_ms"] = round(statistics.median(tk), 4)
    out["min_track_carry_ms"] = round(min(tk), 4)
    out["track_carry_timing"] = f"device events around {GATHER_REPS} back-to-back launches / {GATHER_REPS}, median over the hops"
    for k in carried:
        cols = list(zip(*stats[k]))
        out[f"{k}_per_hop_mean"] = dict(zip(("survivors", "born", "padded", "mean_age"),
                                            [round(statistics.mean(c), 2) for c in cols]))
        out[f"{k}_per_hop_min_max_survivors"] = [min(cols[0]), max(cols[0])]
    if args.warm:
        out["warm_mode"] = args.warm_mode
        out["track_warm_ms"] = round(statistics.median(tw), 4)
        out["min_track_warm_ms"] = round(min(tw), 4)
        for k, it in warm_names.items():
            out[f"{k}_warm_slots_per_hop"] = {"mean": round(statistics.mean(wstats[k]), 2), "min": min(wstats[k]),
                                              "max": max(wstats[k])}
            out[f"{k}_vs_carry_1"] = {"max_abs_pred_tracks_px": wdiff[k][0],
                                      "max_abs_pred_tracks_px_slots_with_one_query": wdiff[k][1],
                                      "max_abs_pose_enc": wdiff[k][2]}
        out["warm_diff_note"] = ("differences between two tracker runs on the same frames under random-init weights, which "
                                 "converge to nothing meaningful: not an accuracy figure")
    out.update({"hops": args.hops, "warmup": args.warmup, "max_abs_pose_enc_diff_query_fn_vs_carry_1": err,
                "pose_enc_diff_note": "a difference between two query sets on the same windows, not an error against ground truth",
                "data": "synthetic (N(0,1) frames); random-init weights: the track statistics say little about real imagery"})
    print(json.dumps(out), flush=True)


def landmark_bench(model, args, dev, cfg):
    """--landmarks (with --fuse --carry): ms per push of PoseStream(fuse, carry) with landmarks on against
    off, the two objects alternating push by push in one process, and the comet_landmark_update launch
    alone on a scratch LandmarkMap fed the hop's own outputs."""
    from comet_amd import loop
    from comet_amd.data import crop_intrinsics
    from comet_amd.models.utils import INTRINSICS
    from comet_amd.stream import LandmarkMap, PoseStream, keypoint_candidates
    T, S, N = args.frames, args.image, args.tracks
    g = torch.Generator(device=dev).manual_seed(1)
    total = T + args.warmup + args.hops - 1
    frames = torch.randn(total, 3, S, S, device=dev, generator=g)
    sp = loop._keypoint_init(cfg, dev)
    R0 = torch.tensor([0.8, 0.2, -0.4, 0.4], device=dev)
    anchor = (R0 / R0.norm(), torch.tensor([331.25, 247.5, 11.375], device=dev), 268.44, 0.5, "AMD")
    intr = crop_intrinsics(INTRINSICS["AMD"], (0, 0, 2 * S, 2 * S), S)
    kw = dict(window=T, stride=1, precision=torch.bfloat16, anchor=anchor, fuse=True, carry=True, carry_tracks=N,
              carry_cell=args.cell, carry_min_score=args.min_score, candidate_fn=keypoint_candidates(sp))
    objs = {True: PoseStream(model, landmarks=True, track_intr=intr, **kw), False: PoseStream(model, **kw)}
    scratch = LandmarkMap(T, 1, 1, N, [intr])
    for o in objs.values():
        assert o.push(frames[:T - 1]) == []
    ta, tb, tc, valid, same = [], [], [], [], True
    for j in range(args.warmup + args.hops):
        i = j + T - 1
        order = (True, False) if j % 2 == 0 else (False, True)  # (neither path always runs first)
        ms, res = {}, {}
        for f in order:
            ms[f], res[f] = _timed(lambda: objs[f].push(frames[i]))
        r = res[True][0]
        tr, fr, ft = r.pred_tracks.float()[None].contiguous(), r.fused_R[None].contiguous(), r.fused_T[None].contiguous()
        ids, src = r.track_ids[None].contiguous(), r.track_src[None].contiguous()
        ms_c, _ = _timed(lambda: [scratch.update([0], tr, fr, ft, ids, src) for _ in range(GATHER_REPS)])
        if j >= args.warmup:
            ta.append(ms[True])
            tb.append(ms[False])
            tc.append(ms_c / GATHER_REPS)
            valid.append(int((r.landmark_state == 1).sum()))
            same = same and torch.equal(r.pred_pose_enc, res[False][0].pred_pose_enc)
    a, b, c = statistics.median(ta), statistics.median(tb), statistics.median(tc)
    print(json.dumps({
        "metric": f"ms per push, landmarks on against off, PoseStream fuse + carry, T={T} {S}^2 N={N}, bf16, stride 1",
        "landmarks_on_ms": round(a, 3), "landmarks_off_ms": round(b, 3), "on_over_off": round(a / b, 4),
        "min_landmarks_on_ms": round(min(ta), 3), "min_landmarks_off_ms": round(min(tb), 3),
        "landmark_update_ms": round(c, 4), "min_landmark_update_ms": round(min(tc), 4),
        "landmark_update_timing": f"device events around {GATHER_REPS} back-to-back launches / {GATHER_REPS}, median over the pushes",
        "valid_landmarks_per_hop": {"mean": round(statistics.mean(valid), 2), "min": min(valid), "max": max(valid)},
        "pred_pose_enc_identical_on_vs_off": same, "pushes": args.hops, "warmup": args.warmup,
        "data": "synthetic (N(0,1) frames, detector candidates); random-init weights: the landmarks carry no geometry"}),
        flush=True)


def pnp_bench(model, args, dev, cfg):
    """--pnp (with --fuse --carry --landmarks): ms per push of PoseStream(fuse, carry, landmarks) with pnp on
    (report only) against off, the two objects alternating push by push in one process, and the
    comet_landmark_pnp launch alone on the hop's own outputs."""
    from comet_amd import loop
    from comet_amd.data import crop_intrinsics
    from comet_amd.models.utils import INTRINSICS
    from comet_amd.ops import LandmarkOut
    from comet_amd.stream import LandmarkMap, PoseStream, keypoint_candidates
    T, S, N = args.frames, args.image, args.tracks
    g = torch.Generator(device=dev).manual_seed(1)
    total = T + args.warmup + args.hops - 1
    frames = torch.randn(total, 3, S, S, device=dev, generator=g)
    sp = loop._keypoint_init(cfg, dev)
    R0 = torch.tensor([0.8, 0.2, -0.4, 0.4], device=dev)
    anchor = (R0 / R0.norm(), torch.tensor([331.25, 247.5, 11.375], device=dev), 268.44, 0.5, "AMD")
    intr = crop_intrinsics(INTRINSICS["AMD"], (0, 0, 2 * S, 2 * S), S)
    kw = dict(window=T, stride=1, precision=torch.bfloat16, anchor=anchor, fuse=True, carry=True, carry_tracks=N,
              carry_cell=args.cell, carry_min_score=args.min_score, candidate_fn=keypoint_candidates(sp),
              landmarks=True, track_intr=intr)
    objs = {True: PoseStream(model, pnp=True, pnp_huber_px=args.pnp_huber_px, **kw), False: PoseStream(model, **kw)}
    scratch = LandmarkMap(T, 1, 1, N, [intr])
    for o in objs.values():
        assert o.push(frames[:T - 1]) == []
    ta, tb, tc, solved, same = [], [], [], [], True
    for j in range(args.warmup + args.hops):
        i = j + T - 1
        order = (True, False) if j % 2 == 0 else (False, True)  # (neither path always runs first)
        ms, res = {}, {}
        for f in order:
            ms[f], res[f] = _timed(lambda: objs[f].push(frames[i]))
        r = res[True][0]
        tr, fr, ft = r.pred_tracks.float()[None].contiguous(), r.fused_R[None].contiguous(), r.fused_T[None].contiguous()
        lo = LandmarkOut(r.landmarks[None].contiguous(), r.landmark_obs[None].contiguous(),
                         r.landmark_err[None].contiguous(), r.landmark_state[None].contiguous())
        ms_c, _ = _timed(lambda: [scratch.pnp([0], tr, fr, ft, lo, huber_px=args.pnp_huber_px) for _ in range(GATHER_REPS)])
        if j >= args.warmup:
            ta.append(ms[True])
            tb.append(ms[False])
            tc.append(ms_c / GATHER_REPS)
            solved.append(int((r.pnp_state == 1).sum()))
            same = same and torch.equal(r.pred_pose_enc, res[False][0].pred_pose_enc)
    a, b, c = statistics.median(ta), statistics.median(tb), statistics.median(tc)
    print(json.dumps({
        "metric": f"ms per push, pnp on against off, PoseStream fuse + carry + landmarks, T={T} {S}^2 N={N}, bf16, stride 1",
        "pnp_on_ms": round(a, 3), "pnp_off_ms": round(b, 3), "on_over_off": round(a / b, 4),
        "min_pnp_on_ms": round(min(ta), 3), "min_pnp_off_ms": round(min(tb), 3),
        "landmark_pnp_ms": round(c, 4), "min_landmark_pnp_ms": round(min(tc), 4),
        "landmark_pnp_timing": f"device events around {GATHER_REPS} back-to-back launches / {GATHER_REPS}, median over the pushes",
        "pnp_iters": 4, "pnp_huber_px": args.pnp_huber_px,
        "solved_positions_per_hop": {"mean": round(statistics.mean(solved), 2), "min": min(solved), "max": max(solved)},
        "pred_pose_enc_identical_on_vs_off": same, "pushes": args.hops, "warmup": args.warmup,
        "data": "synthetic (N(0,1) frames, detector candidates); random-init weights: the poses carry no geometry"}),
        flush=True)


def reid_bench(model, args, dev, cfg):
    """--reid (with --fuse --carry --landmarks): ms per push of PoseStream(fuse, carry, landmarks) with the
    landmark archive on against off, the two objects alternating push by push in one process with the order
    rotating, and the comet_landmark_reid launch alone on the hop's own inputs (on a scratch map, so the
    timed stream's archive is left alone)."""
    from comet_amd import loop
    from comet_amd.data import crop_intrinsics
    from comet_amd.models.utils import INTRINSICS
    from comet_amd.stream import LandmarkMap, PoseStream, keypoint_candidates
    T, S, N = args.frames, args.image, args.tracks
    g = torch.Generator(device=dev).manual_seed(1)
    total = T + args.warmup + args.hops - 1
    frames = torch.randn(total, 3, S, S, device=dev, generator=g)
    sp = loop._keypoint_init(cfg, dev)
    R0 = torch.tensor([0.8, 0.2, -0.4, 0.4], device=dev)
    anchor = (R0 / R0.norm(), torch.tensor([331.25, 247.5, 11.375], device=dev), 268.44, 0.5, "AMD")
    intr = crop_intrinsics(INTRINSICS["AMD"], (0, 0, 2 * S, 2 * S), S)
    kw = dict(window=T, stride=1, precision=torch.bfloat16, anchor=anchor, fuse=True, carry=True, carry_tracks=N,
              carry_cell=args.cell, carry_min_score=args.min_score, candidate_fn=keypoint_candidates(sp),
              landmarks=True, track_intr=intr)
    objs = {True: PoseStream(model, lm_archive=args.reid_capacity, reid_px=args.reid_px, **kw), False: PoseStream(model, **kw)}
    scratch = LandmarkMap(T, 1, 1, N, [intr], archive=args.reid_capacity, reid_px=args.reid_px)
    for o in objs.values():
        assert o.push(frames[:T - 1]) == []
    ta, tb, tc, stats, same = [], [], [], [], True
    for j in range(args.warmup + args.hops):
        i = j + T - 1
        order = (True, False) if j % 2 == 0 else (False, True)  # (neither path always runs first)
        ms, res = {}, {}
        for f in order:
            ms[f], res[f] = _timed(lambda: objs[f].push(frames[i]))
        r = res[True][0]
        tr, fr, ft = r.pred_tracks.float()[None].contiguous(), r.fused_R[None].contiguous(), r.fused_T[None].contiguous()
        ids, src = r.track_ids[None].contiguous(), r.track_src[None].contiguous()
        ms_c, outs = _timed(lambda: [scratch.reidentify([0], tr, fr, ft, ids, src) for _ in range(GATHER_REPS)])
        scratch.update([0], tr, fr, ft, ids, outs[-1].src_lm)  # (the scratch map lives on: its rows die and retire)
        if j >= args.warmup:
            ta.append(ms[True])
            tb.append(ms[False])
            tc.append(ms_c / GATHER_REPS)
            stats.append(objs[True].landmark_map.archive_snapshot(0)[0].numel())
            same = same and torch.equal(r.pred_pose_enc, res[False][0].pred_pose_enc)
    a, b, c = statistics.median(ta), statistics.median(tb), statistics.median(tc)
    print(json.dumps({
        "metric": f"ms per push, landmark archive on against off, PoseStream fuse + carry + landmarks, T={T} {S}^2 N={N} "
                  f"C={args.reid_capacity}, bf16, stride 1",
        "reid_on_ms": round(a, 3), "reid_off_ms": round(b, 3), "on_over_off": round(a / b, 4),
        "min_reid_on_ms": round(min(ta), 3), "min_reid_off_ms": round(min(tb), 3),
        "landmark_reid_ms": round(c, 4), "min_landmark_reid_ms": round(min(tc), 4),
        "landmark_reid_timing": f"device events around {GATHER_REPS} back-to-back launches / {GATHER_REPS}, median over the pushes",
        "reid_px": args.reid_px, "archived_entries": {"mean": round(statistics.mean(stats), 2), "max": max(stats)},
        "pred_pose_enc_identical_on_vs_off": same, "pushes": args.hops, "warmup": args.warmup,
        "data": "synthetic (N(0,1) frames, detector candidates); random-init weights: the landmarks carry no geometry"}),
        flush=True)


def motion_bench(model, args, dev):
    """--motion (with --fuse): ms per push of PoseStream(fuse) with motion on against off, the two objects
    alternating push by push in one process, and the comet_motion_fit launch alone on the hop's own fused
    poses (a scratch tracker: the stream's history is left alone)."""
    from comet_amd.stream import Hop, MotionTracker, PoseStream
    T, S, N = args.frames, args.image, args.tracks
    g = torch.Generator(device=dev).manual_seed(1)
    total = T + args.warmup + args.hops - 1
    frames = torch.randn(total, 3, S, S, device=dev, generator=g)
    q = torch.rand(N, 2, device=dev, generator=g) * (S - 1)
    R0 = torch.tensor([0.8, 0.2, -0.4, 0.4], device=dev)
    anchor = (R0 / R0.norm(), torch.tensor([331.25, 247.5, 11.375], device=dev), 268.44, 0.5, "AMD")
    kw = dict(window=T, stride=1, precision=torch.bfloat16, anchor=anchor, fuse=True)
    objs = {True: PoseStream(model, motion=True, **kw), False: PoseStream(model, **kw)}
    scratch = MotionTracker(T, 1, 1)
    for o in objs.values():
        assert o.push(frames[:T - 1], query_points=q) == []
    ta, tb, tc, states, same = [], [], [], {}, True
    for j in range(args.warmup + args.hops):
        i = j + T - 1
        order = (True, False) if j % 2 == 0 else (False, True)  # (neither path always runs first)
        ms, res = {}, {}
        for f in order:
            ms[f], res[f] = _timed(lambda: objs[f].push(frames[i], query_points=q))
        r, off = res[True][0], res[False][0]
        fused = SimpleNamespace(R=r.fused_R.contiguous(), T=r.fused_T.contiguous())

        def alone():
            for _ in range(GATHER_REPS):  # (reset: the same hop again is a first hop again)
                scratch.reset()
                scratch.update([(0, Hop(r.frame_index, 0))], fused)
        ms_c, _ = _timed(alone)
        if j >= args.warmup:
            ta.append(ms[True])
            tb.append(ms[False])
            tc.append(ms_c / GATHER_REPS)
            st = int(r.motion_state)
            states[st] = states.get(st, 0) + 1
            same = same and torch.equal(r.pred_pose_enc, off.pred_pose_enc) and torch.equal(r.fused_R, off.fused_R) \
                and torch.equal(r.fused_T, off.fused_T)
    a, b, c = statistics.median(ta), statistics.median(tb), statistics.median(tc)
    print(json.dumps({
        "metric": f"ms per push, motion on against off, PoseStream fuse, T={T} {S}^2 N={N}, bf16, stride 1",
        "motion_on_ms": round(a, 3), "motion_off_ms": round(b, 3), "on_over_off": round(a / b, 4),
        "min_motion_on_ms": round(min(ta), 3), "min_motion_off_ms": round(min(tb), 3),
        "motion_fit_ms": round(c, 4), "min_motion_fit_ms": round(min(tc), 4),
        "motion_fit_timing": f"device events around {GATHER_REPS} back-to-back launches / {GATHER_REPS}, median over the "
                             "pushes (a first hop each: one frame in the history)",
        "motion_len": 16, "motion_iters": 2, "states_seen": {str(k): v for k, v in sorted(states.items())},
        "pose_enc_and_fused_poses_identical_on_vs_off": same, "pushes": args.hops, "warmup": args.warmup,
        "data": "synthetic (N(0,1) frames, U[0,S-1] query points); random-init weights: the poses carry no motion"}),
        flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16, help="window length T")
    ap.add_argument("--image", type=int, default=512)
    ap.add_argument("--tracks", type=int, default=512)
    ap.add_argument("--hops", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--streams", type=str, default=None,
                    help="comma-separated stream counts: time StreamPool against that many separate PoseStream objects")
    ap.add_argument("--fuse", action="store_true",
                    help="time pose fusion on against off (PoseStream, or StreamPool with --streams)")
    ap.add_argument("--carry", action="store_true", help="time track carry against the detector on every hop")
    ap.add_argument("--detect-every", type=int, default=4, help="--carry: the detector period of the third stream")
    ap.add_argument("--min-score", type=float, default=0.0, help="--carry: carry_min_score")
    ap.add_argument("--cell", type=int, default=8, help="--carry: carry_cell")
    ap.add_argument("--warm", action="store_true", help="--carry: add warm-started streams to the comparison")
    ap.add_argument("--warm-iters", type=str, default=None,
                    help="--warm: comma-separated coarse iteration counts, one warm stream each (default: the config's)")
    ap.add_argument("--warm-mode", type=str, default="hold", choices=("hold", "velocity"), help="--warm: warm_mode")
    ap.add_argument("--landmarks", action="store_true",
                    help="--fuse --carry: time the landmark map (comet_landmark_update) on against off")
    ap.add_argument("--pnp", action="store_true",
                    help="--fuse --carry --landmarks: time the PnP refinement (comet_landmark_pnp) on against off")
    ap.add_argument("--reid", action="store_true",
                    help="--fuse --carry --landmarks: time the landmark archive (comet_landmark_reid) on against off")
    ap.add_argument("--reid-px", type=float, default=2.0, help="--reid: reid_px (not a recommendation)")
    ap.add_argument("--reid-capacity", type=int, default=4096, help="--reid: lm_archive, entries per stream")
    ap.add_argument("--pnp-huber-px", type=float, default=3.0, help="--pnp: pnp_huber_px (not a recommendation)")
    ap.add_argument("--motion", action="store_true",
                    help="--fuse: time the motion estimate (comet_motion_fit) on against off")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("stream_bench: no GPU", file=sys.stderr)
        return 2
    from comet_amd import functional as F
    from comet_amd import ops
    from comet_amd.config import instantiate, load_config
    from comet_amd.stream import PoseStream
    T, S, N = args.frames, args.image, args.tracks
    dev = torch.device("cuda", 0)
    cfg = load_config()
    torch.manual_seed(0)
    model = instantiate(cfg.MODEL, _recursive_=False, cfg=cfg).to(dev).eval()
    if args.motion:
        if not args.fuse or args.carry or args.streams is not None:
            ap.error("--motion needs --fuse, without --carry and --streams")
        motion_bench(model, args, dev)
        return 0
    if args.warm and not args.carry:
        ap.error("--warm needs --carry")
    if args.landmarks:
        if not (args.fuse and args.carry):
            ap.error("--landmarks needs --fuse --carry")
        if args.pnp:
            pnp_bench(model, args, dev, cfg)
            return 0
        if args.reid:
            reid_bench(model, args, dev, cfg)
            return 0
        landmark_bench(model, args, dev, cfg)
        return 0
    if args.pnp:
        ap.error("--pnp needs --fuse --carry --landmarks")
    if args.reid:
        ap.error("--reid needs --fuse --carry --landmarks")
    if args.carry:
        carry_bench(model, args, dev, cfg)
        return 0
    if args.fuse:
        for n_streams in ([0] if args.streams is None else [int(v) for v in args.streams.split(",")]):
            fuse_bench(model, n_streams, args, dev)
        return 0
    if args.streams is not None:
        for n_streams in [int(v) for v in args.streams.split(",")]:
            pool_bench(model, n_streams, args, dev)
        return 0
    g = torch.Generator(device=dev).manual_seed(1)
    total = T + args.warmup + args.hops - 1
    frames = torch.randn(total, 3, S, S, device=dev, generator=g)
    q = torch.rand(N, 2, device=dev, generator=g) * (S - 1)
    tracks = q[None, None].expand(1, T, N, 2)
    stream = PoseStream(model, window=T, stride=1, precision=torch.bfloat16)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def closed(k):
        with F.precision(torch.bfloat16):
            return model(frames[None, k:k + T], training=False, tracks=tracks)

    stream.push(frames[:T - 1], query_points=q)
    pairs = [(r, w) for r, w in zip(stream._rings, stream._wins) if r is not None]  # the gather of one window
    ta, tb, tc, err = [], [], [], 0.0
    for k in range(args.warmup + args.hops):
        ms_a, res = timed(lambda: stream.push(frames[k + T - 1], query_points=q))
        ms_b, ref = timed(lambda: closed(k))
        assert len(res) == 1 and res[0].frame_index == k
        table = stream._pool._table(stream.sched.window_slots(k % stream.sched.capacity))
        ms_c, _ = timed(lambda: [ops.ring_gather(pairs, *table) for _ in range(GATHER_REPS)])
        ms_c /= GATHER_REPS
        if k >= args.warmup:
            ta.append(ms_a)
            tb.append(ms_b)
            tc.append(ms_c)
            err = max(err, float((res[0].pred_pose_enc - ref["pred_pose_enc"]).abs().max()))
    nbytes = sum(2 * w.numel() * w.element_size() for w in stream._wins if w is not None)
    a, b, c = statistics.median(ta), statistics.median(tb), statistics.median(tc)
    print(json.dumps({
        "metric": f"ms per hop, online COMET inference, T={T} {S}^2 N={N}, bf16, stride 1",
        "stream_ms": round(a, 3), "closed_window_ms": round(b, 3), "gather_ms": round(c, 4),
        "closed_over_stream": round(b / a, 3), "stream_hops_per_s": round(1e3 / a, 2),
        "gather_bytes_read_plus_written": nbytes, "gather_GBps": round(nbytes / (c * 1e-3) / 1e9, 1),
        "gather_timing": f"device events around {GATHER_REPS} back-to-back launches / {GATHER_REPS}, median over the hops",
        "hops": args.hops, "warmup": args.warmup, "min_stream_ms": round(min(ta), 3), "min_closed_ms": round(min(tb), 3),
        "max_abs_pose_enc_diff_stream_vs_closed": err,
        "slot_bytes": {n: (w[0].numel() * w.element_size() if w is not None else 0)
                       for n, w in zip(("fmaps", "frames", "tokens"), stream._wins)},
        "data": "synthetic (N(0,1) frames, U[0,S-1] query points); random-init weights"}))
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
