"""Restatement of the SIFT detector (OpenCV's rules, as DESIGN.md §11 lists them for
comet_amd.keypoints.SIFT) in plain numpy, at a chosen float type. The float64 run is the yardstick of
tests/test_sift_cpu.py and tests/test_sift_gpu.py; the float32 run measures how far a correct
single-precision implementation may sit from it. Nothing here imports the package under test.

Pipeline: uint8 gray -> 2x bilinear up-sample (pixel centres, edge clamp) -> blur to sigma 1.6 ->
per octave nl + 3 Gaussian images (incremental blurs, radius (round(8 sigma + 1) | 1) / 2, taps
normalised in double, reflect-101) -> next octave from every second pixel of layer nl -> DoG
extrema inside a 5-px border, sub-pixel refinement (<= 5 Newton steps), contrast and edge tests,
orientation-histogram peak count -> keep-best-n, filter_dog_point, top-k."""
import functools
import math

import numpy as np

SIGMA = 1.6
BORDER = 5
STEPS = 5
BINS = 36


# ---- images ---------------------------------------------------------------------------------
def synthetic_image(seed, H, W, blobs=40, rects=4):
    """Mid-gray field + Gaussian blobs (std 1.5 .. 6 px, both signs) + a few filled rectangles."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.full((H, W), 128.0)
    for _ in range(rects):
        y0, x0 = rng.integers(4, H - 14), rng.integers(4, W - 14)
        hh, ww = rng.integers(6, max(7, H // 3)), rng.integers(6, max(7, W // 3))
        img[y0:y0 + hh, x0:x0 + ww] += rng.choice([-1.0, 1.0]) * rng.uniform(25, 60)
    for _ in range(blobs):
        cy, cx = rng.uniform(6, H - 6), rng.uniform(6, W - 6)
        s = rng.uniform(1.5, 6.0)
        a = rng.choice([-1.0, 1.0]) * rng.uniform(30, 90)
        img += a * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def blob_image(H, W, cy, cx, s, amp=100.0):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return np.clip(np.rint(100.0 + amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))), 0, 255).astype(np.uint8)


# ---- scale space ----------------------------------------------------------------------------
def reflect101(p, n):
    if n == 1:
        return np.zeros_like(p)
    period = 2 * (n - 1)
    p = np.mod(p, period)
    return np.where(p < n, p, period - p)


def gauss_taps(sigma):
    ks = int(np.rint(sigma * 8 + 1)) | 1
    r = ks // 2
    x = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-x * x / (2.0 * sigma * sigma))
    return w / w.sum(), r


def gauss_blur(img, sigma, dtype):
    """Separable blur of [H, W]; taps rounded to float32 (the table the kernel receives), sums in
    `dtype`, taps in ascending order, rows then columns."""
    w, r = gauss_taps(sigma)
    w = w.astype(np.float32).astype(dtype)
    img = img.astype(dtype)
    H, W = img.shape
    ix = reflect101(np.arange(-r, W + r), W)
    iy = reflect101(np.arange(-r, H + r), H)
    pad = img[:, ix]
    row = np.zeros((H, W), dtype)
    for k in range(2 * r + 1):
        row = row + w[k] * pad[:, k:k + W]
    pad = row[iy, :]
    out = np.zeros((H, W), dtype)
    for k in range(2 * r + 1):
        out = out + w[k] * pad[k:k + H, :]
    return out


def upsample2(gray):
    """2x bilinear, src = (dst + 0.5) / 2 - 0.5, edge-clamped (weights 0.25 / 0.75: exact)."""
    g = gray.astype(np.float64)
    H, W = g.shape

    def axis(n):
        f = (np.arange(2 * n) + 0.5) / 2 - 0.5
        i0 = np.floor(f).astype(int)
        return np.clip(i0, 0, n - 1), np.clip(i0 + 1, 0, n - 1), f - i0

    ya, yb, ly = axis(H)
    xa, xb, lx = axis(W)
    top = g[ya][:, xa] * (1 - lx) + g[ya][:, xb] * lx
    bot = g[yb][:, xa] * (1 - lx) + g[yb][:, xb] * lx
    return top * (1 - ly)[:, None] + bot * ly[:, None]


def base_sigma():
    return math.sqrt(max(SIGMA * SIGMA - (2 * 0.5) ** 2, 0.01))


def layer_sigmas(nl):
    k = 2.0 ** (1.0 / nl)
    return [math.sqrt((SIGMA * k ** i) ** 2 - (SIGMA * k ** (i - 1)) ** 2) for i in range(1, nl + 3)]


def num_octaves(H, W):
    """OpenCV: round(log2(min side of the base image)) - 2) + 1, the base being the 2x up-sample."""
    return int(np.rint(math.log2(min(2 * H, 2 * W)) - 2)) + 1


def pyramid(gray, nl=4, dtype=np.float64):
    """-> list over octaves of [nl + 3, h, w] Gaussian images (every octave, however small)."""
    H, W = gray.shape
    base = gauss_blur(upsample2(gray), base_sigma(), dtype)
    sig = layer_sigmas(nl)
    octs = []
    for o in range(num_octaves(H, W)):
        layers = [base]
        for i in range(1, nl + 3):
            layers.append(gauss_blur(layers[-1], sig[i - 1], dtype))
        octs.append(np.stack(layers))
        h, w = base.shape
        if h < 2 or w < 2:
            break
        base = layers[nl][0:2 * (h // 2):2, 0:2 * (w // 2):2]
    return octs


# ---- detection ------------------------------------------------------------------------------
def solve3(Hm, g, dtype):
    """x with Hm x = -g: Gaussian elimination with partial pivoting in `dtype`; None when singular."""
    A = np.concatenate([Hm.astype(dtype), -g.astype(dtype)[:, None]], 1)
    for c in range(3):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        if A[p, c] == 0:
            return None
        if p != c:
            A[[c, p]] = A[[p, c]]
        for q in range(c + 1, 3):
            f = A[q, c] / A[c, c]
            A[q, c + 1:] = A[q, c + 1:] - f * A[c, c + 1:]
    x2 = A[2, 3] / A[2, 2]
    x1 = (A[1, 3] - A[1, 2] * x2) / A[1, 1]
    x0 = (A[0, 3] - A[0, 1] * x1 - A[0, 2] * x2) / A[0, 0]
    return np.array([x0, x1, x2], dtype)


def orientation_count(img, r, c, scl, dtype):
    h, w = img.shape
    rad = int(np.rint(dtype(4.5) * scl))
    sg = dtype(1.5) * scl
    es = dtype(-1.0) / (dtype(2.0) * sg * sg)
    hist = np.zeros(BINS, dtype)
    for i in range(-rad, rad + 1):
        y = r + i
        if y <= 0 or y >= h - 1:
            continue
        for j in range(-rad, rad + 1):
            x = c + j
            if x <= 0 or x >= w - 1:
                continue
            dx = img[y, x + 1] - img[y, x - 1]
            dy = img[y - 1, x] - img[y + 1, x]
            wgt = np.exp(dtype(i * i + j * j) * es)
            ang = np.arctan2(dy, dx) * dtype(180.0 / math.pi)
            if ang < 0:
                ang += dtype(360.0)
            b = int(np.rint(ang * dtype(BINS / 360.0)))
            b = b - BINS if b >= BINS else b
            b = b + BINS if b < 0 else b
            hist[b] += wgt * np.sqrt(dx * dx + dy * dy)
    t = hist
    sm = (np.roll(t, 2) + np.roll(t, -2)) * dtype(1 / 16) + (np.roll(t, 1) + np.roll(t, -1)) * dtype(4 / 16) + t * dtype(6 / 16)
    mx = sm.max()
    peak = (sm > np.roll(sm, 1)) & (sm > np.roll(sm, -1)) & (sm >= dtype(0.8) * mx)
    return int(peak.sum())


def detect(gray, nl=4, contrast_threshold=0.0066667, edge_threshold=10.0, dtype=np.float64, octaves=None):
    """-> list of dicts, one per keypoint before any cut: x, y, size (pixels of `gray`), response,
    nori, octave, layer, r, c (integer sample of the octave) and the margins that say how close each
    decision was (contrast ratio, edge ratio, largest |offset|, 26-neighbour margin in gray levels)."""
    dtype = np.dtype(dtype).type
    octs = pyramid(gray, nl, dtype) if octaves is None else octaves
    thr = math.floor(0.5 * contrast_threshold / nl * 255)
    ct, et = dtype(contrast_threshold), dtype(edge_threshold)
    ds, d2s, dcs = dtype(0.5 / 255), dtype(1.0 / 255), dtype(0.25 / 255)
    out = []
    for o, G in enumerate(octs):
        D = G[1:] - G[:-1]
        _, h, w = D.shape
        if h <= 2 * BORDER or w <= 2 * BORDER:
            continue
        for s in range(1, nl + 1):
            ctr = D[s, BORDER:h - BORDER, BORDER:w - BORDER]
            nb = np.stack([D[s + k, BORDER + dy:h - BORDER + dy, BORDER + dx:w - BORDER + dx]
                           for k in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
            is_max = (ctr > 0) & (ctr >= nb).all(0)
            is_min = (ctr < 0) & (ctr <= nb).all(0)
            ys, xs = np.nonzero((np.abs(ctr) > thr) & (is_max | is_min))
            for r0, c0 in zip(ys + BORDER, xs + BORDER):
                v0 = D[s, r0, c0]
                cube = D[s - 1:s + 2, r0 - 1:r0 + 2, c0 - 1:c0 + 2].copy()
                cube[1, 1, 1] = -np.inf if v0 > 0 else np.inf
                margin = float(v0 - cube.max()) if v0 > 0 else float(cube.min() - v0)
                r, c, l = int(r0), int(c0), s
                kp = None
                for _ in range(STEPS):
                    v2 = dtype(2) * D[l, r, c]
                    cxp, cxm, cyp, cym = D[l, r, c + 1], D[l, r, c - 1], D[l, r + 1, c], D[l, r - 1, c]
                    nx, pv = D[l + 1, r, c], D[l - 1, r, c]
                    g = np.array([(cxp - cxm) * ds, (cyp - cym) * ds, (nx - pv) * ds], dtype)
                    dxx, dyy, dss = (cxp + cxm - v2) * d2s, (cyp + cym - v2) * d2s, (nx + pv - v2) * d2s
                    dxy = (D[l, r + 1, c + 1] - D[l, r + 1, c - 1] - D[l, r - 1, c + 1] + D[l, r - 1, c - 1]) * dcs
                    dxs = (D[l + 1, r, c + 1] - D[l + 1, r, c - 1] - D[l - 1, r, c + 1] + D[l - 1, r, c - 1]) * dcs
                    dys = (D[l + 1, r + 1, c] - D[l + 1, r - 1, c] - D[l - 1, r + 1, c] + D[l - 1, r - 1, c]) * dcs
                    Hm = np.array([[dxx, dxy, dxs], [dxy, dyy, dys], [dxs, dys, dss]], dtype)
                    X = solve3(Hm, g, dtype)
                    if X is None:
                        break
                    xc, xr, xi = X
                    if abs(xc) < 0.5 and abs(xr) < 0.5 and abs(xi) < 0.5:
                        contr = dtype(0.5) * v2 * d2s + dtype(0.5) * (g[0] * xc + g[1] * xr + g[2] * xi)
                        tr, det = dxx + dyy, dxx * dyy - dxy * dxy
                        if abs(contr) * dtype(nl) >= ct and det > 0 and tr * tr * et < (et + 1) * (et + 1) * det:
                            scl = dtype(SIGMA) * np.exp2((dtype(l) + xi) / dtype(nl))
                            osc = dtype(2 ** o)
                            kp = dict(x=float((dtype(c) + xc) * osc) * 0.5, y=float((dtype(r) + xr) * osc) * 0.5,
                                      size=float(scl * osc * dtype(2)) * 0.5, response=float(abs(contr)),
                                      octave=o, layer=l, r=r, c=c,
                                      nori=orientation_count(G[l], r, c, scl, dtype),
                                      m_contrast=float(abs(contr) * dtype(nl) / ct),
                                      m_edge=float(tr * tr * et / ((et + 1) * (et + 1) * det)),
                                      m_offset=float(max(abs(xc), abs(xr), abs(xi))), m_extremum=margin)
                        break
                    if not (abs(xc) < 1e6 and abs(xr) < 1e6 and abs(xi) < 1e6):
                        break
                    c += int(np.rint(xc))
                    r += int(np.rint(xr))
                    l += int(np.rint(xi))
                    if l < 1 or l > nl or c < BORDER or c >= w - BORDER or r < BORDER or r >= h - BORDER:
                        break
                if kp is not None:
                    out.append(kp)
    out.sort(key=lambda k: (-k["response"], k["octave"], k["layer"], k["y"], k["x"]))
    return out


def is_marginal(k):
    """A float64 keypoint whose acceptance hangs on a near-tie: a single-precision run may differ."""
    return (k["m_contrast"] < 1.05 or k["m_edge"] > 0.95 or k["m_offset"] > 0.48 or k["m_extremum"] < 1e-3)


def match(ref, other):
    """For every keypoint of `ref` the nearest keypoint of `other` in the same octave and layer
    within 1 px of the octave's grid (None when there is none) -> list of indices into `other`."""
    res = []
    for k in ref:
        best, bd = None, None
        for j, q in enumerate(other):
            if q["octave"] != k["octave"] or q["layer"] != k["layer"]:
                continue
            d = math.hypot(q["x"] - k["x"], q["y"] - k["y"])
            if d <= 0.5 * 2 ** k["octave"] and (bd is None or d < bd):
                best, bd = j, d
        res.append(best)
    return res


# ---- selection ------------------------------------------------------------------------------
def select(x, y, resp, nori, H, W, max_num, nms_radius=0):
    """Indices (into lists sorted by response, best first) that survive OpenCV's keep-best-n over the
    orientation-expanded list (ties with the last kept response stay), filter_dog_point (best score
    per rounded pixel, first of the list on equal scores; (2 r + 1)^2 max filter) and the top-k."""
    x, y, resp, nori = (np.asarray(a, np.float64) for a in (x, y, resp, nori))
    idx = np.nonzero(nori > 0)[0]
    if max_num is not None and idx.size and nori[idx].sum() > max_num:
        expanded = np.repeat(resp[idx], nori[idx].astype(int))
        last = np.sort(expanded)[::-1][max_num - 1]
        idx = idx[resp[idx] >= last]
    ix = np.clip(np.round(x[idx] - 0.5).astype(int), 0, W - 1)
    iy = np.clip(np.round(y[idx] - 0.5).astype(int), 0, H - 1)
    seen, keep = set(), []
    for n, (a, b) in enumerate(zip(iy, ix)):
        if (a, b) not in seen:
            seen.add((a, b))
            keep.append(n)
    idx, iy, ix = idx[keep], iy[keep], ix[keep]
    if nms_radius > 0:
        buf = np.zeros((H, W))
        buf[iy, ix] = resp[idx]
        ok = []
        for n, (a, b) in enumerate(zip(iy, ix)):
            win = buf[max(a - nms_radius, 0):a + nms_radius + 1, max(b - nms_radius, 0):b + nms_radius + 1]
            if buf[a, b] == win.max():
                ok.append(n)
        idx = idx[ok]
    if max_num is not None and idx.size > max_num:
        idx = idx[:max_num]
    return idx


# ---- the shared test inputs and the noise floor ----------------------------------------------
SEED = 76
SHAPES = ((64, 64), (97, 83))


@functools.lru_cache(maxsize=None)
def images():
    """B = 2 images per shape -> {(H, W): uint8 [2, H, W]}."""
    return {hw: np.stack([synthetic_image(SEED + 100 * n + i, *hw) for i in range(2)]) for n, hw in enumerate(SHAPES)}


@functools.lru_cache(maxsize=None)
def reference():
    """float64 and float32 runs on every test image and the float32-vs-float64 floors.
    -> {"kp64": {(H, W): [list, list]}, "kp32": ..., "pyr64": ..., "floor": {image, pos, size, response}}."""
    kp64, kp32, pyr64 = {}, {}, {}
    f_img = f_pos = f_size = f_resp = 0.0
    for hw, imgs in images().items():
        kp64[hw], kp32[hw], pyr64[hw] = [], [], []
        for g in imgs:
            p64, p32 = pyramid(g, 4, np.float64), pyramid(g, 4, np.float32)
            f_img = max(f_img, max(float(np.abs(a - b).max()) for a, b in zip(p64, p32)))
            k64 = detect(g, dtype=np.float64, octaves=p64)
            k32 = detect(g, dtype=np.float32, octaves=p32)
            for k, j in zip(k64, match(k64, k32)):
                if j is None or is_marginal(k):
                    continue
                q = k32[j]
                f_pos = max(f_pos, abs(q["x"] - k["x"]), abs(q["y"] - k["y"]))
                f_size = max(f_size, abs(q["size"] - k["size"]))
                f_resp = max(f_resp, abs(q["response"] - k["response"]))
            kp64[hw].append(k64)
            kp32[hw].append(k32)
            pyr64[hw].append(p64)
    return {"kp64": kp64, "kp32": kp32, "pyr64": pyr64,
            "floor": {"image": f_img, "pos": f_pos, "size": f_size, "response": f_resp}}
