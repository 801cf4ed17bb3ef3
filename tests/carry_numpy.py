"""A plain numpy restatement of comet_track_carry (include/comet_hip.h, DESIGN.md "Track carry"),
rules 1-5, with sequential loops: the pin for the kernel. No torch, no GPU.

Every output is a copy of an input or an integer, so the comparison with the kernel is equality. The
one exception is the lattice pad (rule 5, L == 0), which both sides compute in float32 with the same
expression, evaluated left to right, one rounding per operation:

    g = ceil(sqrt(N))                                    (exact, in integers)
    x = (float32(r % g) + float32(0.5)) * float32(W) / float32(g)
    y = (float32(r // g) + float32(0.5)) * float32(H) / float32(g)

The cell of a point is floor(float32(x) / float32(cell)) in float32, likewise for y; the mask is read
at (clamp(rint(y), 0, H - 1), clamp(rint(x), 0, W - 1)) with rint rounding half to even."""
import numpy as np

INT32_MIN = -2 ** 31
INT32_MAX = 2 ** 31 - 1
AGE_MAX = 2 ** 19 - 1
f32 = np.float32


def isqrt_ceil(n):
    g = 1
    while g * g < n:
        g += 1
    return g


def alive(x, y, H, W, cell, border, mask):
    """Rule 1 for a position -> (alive, cell index (cx, cy))."""
    x, y = f32(x), f32(y)
    if not (np.isfinite(x) and np.isfinite(y)):
        return False, None
    if not (f32(border) <= x <= f32(W - 1 - border) and f32(border) <= y <= f32(H - 1 - border)):
        return False, None
    if mask is not None:
        ix = min(max(int(np.rint(x)), 0), W - 1)
        iy = min(max(int(np.rint(y)), 0), H - 1)
        if mask[iy, ix] == 0:
            return False, None
    return True, (int(np.floor(x / f32(cell))), int(np.floor(y / f32(cell))))


def track_key(age, j):
    return ((AGE_MAX - min(max(int(age), 0), AGE_MAX)) << 12) | j


def carry_one(tracks, score, ids, age, mask, cand, cand_n, next_id, prev_valid, s, H, W, cell, border, min_score):
    """One hop. tracks [T, N, 2] f32, score [T, N] f32, ids / age [N] int32, mask [H, W] uint8 or None,
    cand [M, 2] f32 or None -> (query [N, 2] f32, ids [N], age [N], src [N] (int32), stats [4], next_id)."""
    N = ids.shape[0]
    gw, gh = -(-W // cell), -(-H // cell)
    cn = 0 if cand is None else min(max(int(cand_n), 0), cand.shape[0])
    min_score = f32(min_score)
    cells = {}  # (cx, cy) -> minimum key
    tcell, ccell = [None] * N, [None] * cn
    if prev_valid:
        for j in range(N):
            if ids[j] < 0 or not (f32(score[s, j]) >= min_score):
                continue
            ok, c = alive(tracks[s, j, 0], tracks[s, j, 1], H, W, cell, border, mask)
            if ok:
                assert 0 <= c[0] < gw and 0 <= c[1] < gh
                tcell[j] = c
                cells[c] = min(cells.get(c, 2 ** 32), track_key(age[j], j))
    for c in range(cn):
        ok, g = alive(cand[c, 0], cand[c, 1], H, W, cell, border, mask)
        if ok:
            assert 0 <= g[0] < gw and 0 <= g[1] < gh
            ccell[c] = g
            cells[g] = min(cells.get(g, 2 ** 32), (1 << 31) | c)

    query = np.zeros((N, 2), np.float32)
    ids_out = np.zeros(N, np.int32)
    age_out = np.zeros(N, np.int32)
    src = np.zeros(N, np.int32)
    state = [0] * N  # 0 free, 1 kept, 2 born
    survivors = dropped = 0
    for j in range(N):
        if tcell[j] is None:
            continue
        if cells[tcell[j]] == track_key(age[j], j):
            query[j] = tracks[s, j]
            ids_out[j] = ids[j]
            age_out[j] = min(max(int(age[j]), 0), INT32_MAX - 1) + 1
            src[j] = j
            state[j] = 1
            survivors += 1
        else:
            dropped += 1
    kept_c = [c for c in range(cn) if ccell[c] is not None and cells[ccell[c]] == ((1 << 31) | c)]
    free = [j for j in range(N) if state[j] == 0]
    born = min(len(kept_c), len(free))
    for r in range(born):
        j, c = free[r], kept_c[r]
        query[j] = cand[c]
        ids_out[j] = next_id + r
        age_out[j] = 0
        src[j] = -1 - c
        state[j] = 2
    live = [j for j in range(N) if state[j] != 0]
    L = len(live)
    g = isqrt_ceil(N)
    pads = [j for j in range(N) if state[j] == 0]
    for r, j in enumerate(pads):
        if L > 0:
            k = live[r % L]
            query[j] = query[k]
            src[j] = INT32_MIN + k
        else:
            query[j, 0] = (f32(r % g) + f32(0.5)) * f32(W) / f32(g)
            query[j, 1] = (f32(r // g) + f32(0.5)) * f32(H) / f32(g)
            src[j] = INT32_MIN
        ids_out[j] = -1
        age_out[j] = 0
    stats = np.array([survivors, born, len(pads), dropped], np.int32)
    return query, ids_out, age_out, src, stats, next_id + born


def carry(tracks, score, ids, age, mask, cand, cand_n, next_id, prev_valid, s, H, W, cell, border, min_score):
    """All n hops of a launch: the arguments of comet_track_carry as numpy arrays ([n, ...]; mask and
    cand may be None) -> dict of query, ids, age, src, stats, next_id."""
    n = ids.shape[0]
    outs = [carry_one(tracks[b], score[b], ids[b], age[b], None if mask is None else mask[b],
                      None if cand is None else cand[b], 0 if cand is None else cand_n[b], int(next_id[b]),
                      int(prev_valid[b]), s, H, W, cell, border, min_score) for b in range(n)]
    names = ("query", "ids", "age", "src", "stats")
    out = {k: np.stack([o[i] for o in outs]) for i, k in enumerate(names)}
    out["next_id"] = np.array([o[5] for o in outs], np.int32)
    return out


def random_inputs(seed, n, T, N, M, H, W, s=1, fill=0.7, with_mask=True, spread=1.0):
    """Random launch arguments (a dict of the keyword arguments of `carry`, without the scalars cell,
    border and min_score): positions over a frame enlarged by 4 px on every side (so some lie outside
    it), scores in [0, 1], about `fill` of the slots holding a track with ages 0 .. 5, a mask with a
    blanked rectangle, cand_n between M / 2 and M. spread < 1 crowds the points into a corner (many
    per cell)."""
    rng = np.random.default_rng(seed)
    tracks = (rng.random((n, T, N, 2)) * np.array([W + 8, H + 8]) * spread - 4).astype(np.float32)
    score = rng.random((n, T, N)).astype(np.float32)
    ids = np.where(rng.random((n, N)) < fill, rng.permuted(np.tile(np.arange(N), (n, 1)), axis=1), -1).astype(np.int32)
    age = rng.integers(0, 6, (n, N)).astype(np.int32)
    mask = None
    if with_mask:
        mask = np.ones((n, H, W), np.uint8)
        for b in range(n):
            y0, x0 = rng.integers(0, H // 2), rng.integers(0, W // 2)
            mask[b, y0:y0 + H // 4, x0:x0 + W // 4] = 0
    cand = cand_n = None
    if M > 0:
        cand = (rng.random((n, M, 2)) * np.array([W + 8, H + 8]) * spread - 4).astype(np.float32)
        cand_n = rng.integers(M // 2, M + 1, n).astype(np.int32)
    return dict(tracks=tracks, score=score, ids=ids, age=age, mask=mask, cand=cand, cand_n=cand_n,
                next_id=np.full(n, N, np.int32), prev_valid=np.ones(n, np.int32), s=s, H=H, W=W)
