"""A plain numpy restatement of comet_track_warm (include/comet_hip.h, DESIGN.md "Warm start") with
sequential loops: the pin for the kernel. No torch, no GPU.

Every output value is a copy of an input, or float32 arithmetic both sides evaluate alike, one
rounding per operation and left to right:

    velocity:  v = last + float32(e) * (last - before)        then  v < 0 ? 0 : (v > hi ? hi : v)
    units:     v / float32(div0) / float32(div1)

so the comparison with the kernel is equality of bits."""
import numpy as np

INT32_MIN = -2 ** 31
f32 = np.float32
HOLD, VELOCITY = 0, 1


def donor(src, j, N, prev_valid):
    """The slot of the previous window that slot j continues -> (k or None, warm code 0 / 1 / 2)."""
    if not prev_valid:
        return None, 0
    v = int(src[j])
    if 0 <= v < N:
        return v, 1
    l = v - INT32_MIN
    if 0 <= l < N and int(src[l]) == l:
        return l, 2
    return None, 0


def clamp(v, hi):
    return f32(0) if v < f32(0) else (hi if v > hi else v)


def warm_row(prev, k, q, s, H, W, mode):
    """The warm row of donor k in pixels -> (row [T, 2] f32 after the clamp, whether all its 2 T values
    were finite before it). prev [T, N, 2] f32, q [2] f32."""
    T = prev.shape[0]
    overlap = T - 1 - s
    row = np.zeros((T, 2), np.float32)
    finite = True
    hi = (f32(W - 1), f32(H - 1))
    for i in range(T):
        for c in range(2):
            if i == 0:
                v = f32(q[c])
            elif i <= overlap:
                v = f32(prev[i + s, k, c])
            else:
                last = f32(prev[T - 1, k, c])
                if mode == HOLD:
                    v = last
                else:
                    before = f32(prev[T - 2, k, c])
                    with np.errstate(all="ignore"):
                        d = f32(last - before)
                        v = f32(last + f32(f32(i - overlap) * d))
            if not np.isfinite(v):
                finite = False
            elif i > overlap and mode == VELOCITY:
                v = clamp(v, hi[c])
            row[i, c] = v
    return row, finite


def warm_one(prev, src, query, prev_valid, s, H, W, mode, div0, div1):
    """One hop. prev [T, N, 2] f32, src [N] int32, query [N, 2] f32 -> (coords [N, T, 2] f32, warm [N] int32)."""
    T, N = prev.shape[:2]
    coords = np.zeros((N, T, 2), np.float32)
    warm = np.zeros(N, np.int32)
    d0, d1 = f32(div0), f32(div1)
    for j in range(N):
        k, code = donor(src, j, N, prev_valid)
        row = None
        if k is not None:
            row, finite = warm_row(prev, k, query[j], s, H, W, mode)
            if not finite:
                row, code = None, -1
        if row is None:
            row = np.repeat(query[j][None].astype(np.float32), T, 0)
        for i in range(T):
            for c in range(2):
                with np.errstate(all="ignore"):
                    coords[j, i, c] = f32(f32(row[i, c] / d0) / d1)
        warm[j] = code
    return coords, warm


def warm(prev, src, query, prev_valid, s, H, W, mode, div0, div1):
    """All n hops of a launch: the arguments of comet_track_warm as numpy arrays ([n, ...]) ->
    (coords [n, N, T, 2] f32, warm [n, N] int32)."""
    assert mode in (HOLD, VELOCITY) and 1 <= s <= prev.shape[1] - 1
    outs = [warm_one(prev[b], src[b], query[b], int(prev_valid[b]), s, H, W, mode, div0, div1)
            for b in range(src.shape[0])]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])
