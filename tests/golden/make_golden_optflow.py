#!/usr/bin/env python3
"""Generates tests/golden/optflow_v1.npz -- known answers for FilterOpticalFlow (the reference's
video/filters.py:572-589): cv2.calcOpticalFlowFarneback(prev, next, 0.5, 3, 2, 3, 5, 1.2, 0) and the
magnitude of cv2.cartToPolar.

    python tests/golden/make_golden_optflow.py

Source of truth: the NumPy restatement below of OpenCV's calcOpticalFlowFarneback with flags = 0
(modules/video/src/optflowgf.cpp, its scalar code), one array operation per scalar operation, with
explicit float32 / float64 types and no fused multiply-add anywhere ("Optical flow"). The
two resizes of the algorithm go through the oracle's C restatement of cv2.resize (oracle.resize_f32).
Host constants use Python floats and libm's exp (math.exp).  OpenCV is not needed; where it is
installed, tests/test_gpu_optflow_cv2.py compares the GPU with it.

Importable: tests/test_optflow_host.py checks the restatement against the committed fixture and
tests/test_gpu_optflow.py restates random cases at run time.
"""
import hashlib
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "optflow_v1.npz")
F32, F64 = np.float32, np.float64
FLT_EPSILON = float(np.finfo(np.float32).eps)
MIN_SIZE = 32
# getGaussianKernel's fixed small kernels (sigma <= 0)
_FIXED_TAPS = {1: [1.0], 3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625],
               7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}
_BORDER = np.array([0.14, 0.14, 0.4472, 0.4472, 0.4472], F32)
REFERENCE_PARAMS = dict(pyr_scale=0.5, levels=3, winsize=2, iterations=3, poly_n=5, poly_sigma=1.2)


def _oracle():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import oracle as O
    O.build()
    return O


# ---------------------------------------------------------------------------- step 1: levels
def cv_round(v):
    """cvRound: round half to even"""
    return int(round(float(v)))


def level_plan(h, w, pyr_scale, levels):
    """[(k, scale, sigma, ksize, level_h, level_w)] from the coarsest level down to level 0"""
    scale, k = 1.0, 0
    while k < levels:
        scale *= pyr_scale
        if w * scale < MIN_SIZE or h * scale < MIN_SIZE:
            break
        k += 1
    plan = []
    for k in range(k, -1, -1):
        scale = 1.0
        for _ in range(k):
            scale *= pyr_scale
        sigma = (1.0 / scale - 1) * 0.5
        ksize = max(cv_round(5 * sigma) | 1, 3)
        plan.append((k, scale, sigma, ksize, cv_round(h * scale), cv_round(w * scale)))
    return plan


# ---------------------------------------------------------------------------- step 2: pyramid image
def gauss_taps(ksize, sigma):
    """getGaussianKernel(ksize, sigma, CV_32F)"""
    if sigma <= 0 and ksize <= 7:
        return np.array(_FIXED_TAPS[ksize], F32)
    n = ksize                                   # taps_f64 of va_gauss.hip (getGaussianKernelBitExact)
    n2 = (n - 1) // 2
    scale2x = -0.125 / (sigma * sigma)
    out = [0.0] * n
    s = 0.0
    x = 1 - n
    for i in range(n2):
        out[i] = math.exp(float(x * x) * scale2x)
        s += out[i]
        x += 2
    s *= 2.0
    s += 1.0
    mul1 = 1.0 / s
    for i in range(n2):
        t = out[i] * mul1
        out[i] = t
        out[n - 1 - i] = t
    out[n2] = 1.0 * mul1
    return np.array(out, F64).astype(F32)


def reflect101(idx, n):
    idx = np.array(idx)
    if n == 1:
        return np.zeros_like(idx)
    while (idx < 0).any() or (idx >= n).any():
        idx = np.where(idx < 0, -idx, idx)
        idx = np.where(idx >= n, 2 * (n - 1) - idx, idx)
    return idx


def gaussian_blur(img, taps):
    """GaussianBlur(img, (k, k), sigma) on a float32 (h, w) image, BORDER_REFLECT_101"""
    h, w = img.shape
    k = len(taps)
    r = k // 2
    S = img[:, reflect101(np.arange(-r, w + r), w)]
    col = lambda d: S[:, r + d:r + d + w]
    if k <= 5:                                  # SymmRowSmallFilter
        t = col(0) * taps[r] + (col(-1) + col(1)) * taps[r + 1]
        if k == 5:
            t = t + (col(-2) + col(2)) * taps[r + 2]
    else:                                       # RowFilter
        t = taps[0] * col(-r)
        for i in range(1, k):
            t = t + taps[i] * col(i - r)
    T = t[reflect101(np.arange(-r, h + r), h)]
    row = lambda d: T[r + d:r + d + h]
    s = taps[r] * row(0)                        # SymmColumnFilter
    for j in range(1, r + 1):
        s = s + taps[r + j] * (row(j) + row(-j))
    return s


def resize_linear(img, lh, lw):
    """cv2.resize(img, (lw, lh), INTER_LINEAR): a copy at equal size, else the oracle's restatement"""
    if img.shape[:2] == (lh, lw):
        return img.copy()
    O = _oracle()
    if img.ndim == 2:
        return O.resize_f32(img, (lw, lh), "linear")
    return O.resize_f32(img[None], (lw, lh), "linear")[0]


def pyramid_image(frame32, ksize, sigma, lh, lw):
    return resize_linear(gaussian_blur(frame32, gauss_taps(ksize, sigma)), lh, lw)


# ---------------------------------------------------------------------------- step 3: constants
def poly_consts(n, sigma):
    """FarnebackPrepareGaussian: g, xg, xxg (float32, indices -n..n at 0..2n) and ig11, ig03, ig33, ig55"""
    if sigma < FLT_EPSILON:
        sigma = n * 0.3
    xs = range(-n, n + 1)
    g = {x: F32(math.exp(-x * x / (2 * sigma * sigma))) for x in xs}
    s = 0.0
    for x in xs:
        s += float(g[x])
    s = 1.0 / s
    for x in xs:
        g[x] = F32(float(g[x]) * s)
    xg = {x: F32(x) * g[x] for x in xs}
    xxg = {x: F32(x * x) * g[x] for x in xs}
    G = [[0.0] * 6 for _ in range(6)]
    for y in xs:
        for x in xs:
            gg = g[y] * g[x]
            fx, fy = F32(x), F32(y)
            G[0][0] += float(gg)
            G[1][1] += float(gg * fx * fx)
            G[3][3] += float(gg * fx * fx * fx * fx)
            G[5][5] += float(gg * fx * fx * fy * fy)
    G[2][2] = G[0][3] = G[0][4] = G[3][0] = G[4][0] = G[1][1]
    G[4][4] = G[3][3]
    G[3][4] = G[4][3] = G[5][5]
    inv = cholesky_inverse(G)
    arr = lambda d: np.array([d[x] for x in xs], F32)
    return arr(g), arr(xg), arr(xxg), (inv[1][1], inv[0][3], inv[3][3], inv[5][5])


def cholesky_inverse(A):
    """OpenCV's CholImpl against the identity (Mat::inv(DECOMP_CHOLESKY)), in double"""
    m = len(A)
    L = [row[:] for row in A]
    for i in range(m):
        for j in range(i):
            s = A[i][j]
            for k in range(j):
                s -= L[i][k] * L[j][k]
            L[i][j] = s * L[j][j]
        s = A[i][i]
        for k in range(i):
            t = L[i][k]
            s -= t * t
        if s < sys.float_info.epsilon:
            raise ValueError("G is not positive definite")
        L[i][i] = 1.0 / math.sqrt(s)
    b = [[1.0 if i == j else 0.0 for j in range(m)] for i in range(m)]
    for i in range(m):
        for j in range(m):
            s = b[i][j]
            for k in range(i):
                s -= L[i][k] * b[k][j]
            b[i][j] = s * L[i][i]
    for i in range(m - 1, -1, -1):
        for j in range(m):
            s = b[i][j]
            for k in range(m - 1, i, -1):
                s -= L[k][i] * b[k][j]
            b[i][j] = s * L[i][i]
    return b


# ---------------------------------------------------------------------------- step 4: PolyExp
def poly_exp(I, n, consts):
    """FarnebackPolyExp: R (h, w, 5) float32 of a float32 (h, w) image"""
    g, xg, xxg, (ig11, ig03, ig33, ig55) = consts
    h, w = I.shape
    c = n                                        # index of offset 0 in g / xg / xxg
    rows = lambda k: I[np.clip(np.arange(h) + k, 0, h - 1)]
    t0 = I * g[c]
    t1 = np.zeros_like(I)
    t2 = np.zeros_like(I)
    for k in range(1, n + 1):
        sm, sp = rows(-k), rows(k)
        p = sm + sp
        t0 = t0 + g[c + k] * p
        t1 = t1 + xg[c + k] * (sp - sm)
        t2 = t2 + xxg[c + k] * p
    cols = lambda t, k: t[:, np.clip(np.arange(w) + k, 0, w - 1)]
    b1 = (t0 * g[c]).astype(F64)
    b3 = (t1 * g[c]).astype(F64)
    b5 = (t2 * g[c]).astype(F64)
    b2 = np.zeros((h, w), F64)
    b4 = np.zeros((h, w), F64)
    b6 = np.zeros((h, w), F64)
    for k in range(1, n + 1):
        p0, m0 = cols(t0, k), cols(t0, -k)
        p1, m1 = cols(t1, k), cols(t1, -k)
        p2, m2 = cols(t2, k), cols(t2, -k)
        tg = (p0 + m0).astype(F64)
        b1 = b1 + tg * F64(g[c + k])
        b4 = b4 + tg * F64(xxg[c + k])
        b2 = b2 + ((p0 - m0) * xg[c + k]).astype(F64)
        b3 = b3 + ((p1 + m1) * g[c + k]).astype(F64)
        b6 = b6 + ((p1 - m1) * xg[c + k]).astype(F64)
        b5 = b5 + ((p2 + m2) * g[c + k]).astype(F64)
    return np.stack([(b3 * ig11).astype(F32), (b2 * ig11).astype(F32), (b1 * ig03 + b5 * ig33).astype(F32),
                     (b1 * ig03 + b4 * ig33).astype(F32), (b6 * ig55).astype(F32)], -1)


# ---------------------------------------------------------------------------- step 6: UpdateMatrices
def update_matrices(R0, R1, flow):
    """FarnebackUpdateMatrices over the whole level: M (h, w, 5) float32"""
    h, w = flow.shape[:2]
    dx, dy = flow[..., 0], flow[..., 1]
    X = np.arange(w)[None, :]
    Y = np.arange(h)[:, None]
    fx = X.astype(F32) + dx
    fy = Y.astype(F32) + dy
    x1, y1 = np.floor(fx), np.floor(fy)
    fx = fx - x1
    fy = fy - y1
    inside = (x1 >= 0) & (x1 < w - 1) & (y1 >= 0) & (y1 < h - 1)
    xi = np.where(inside, x1, 0).astype(np.int64)
    yi = np.where(inside, y1, 0).astype(np.int64)
    one = F32(1)
    a00, a01 = (one - fx) * (one - fy), fx * (one - fy)
    a10, a11 = (one - fx) * fy, fx * fy
    s = [a00[..., None] * R1[yi, xi], a01[..., None] * R1[yi, xi + 1],
         a10[..., None] * R1[yi + 1, xi], a11[..., None] * R1[yi + 1, xi + 1]]
    r = ((s[0] + s[1]) + s[2]) + s[3]
    half, quarter = F32(0.5), F32(0.25)
    r2 = np.where(inside, r[..., 0], F32(0))
    r3 = np.where(inside, r[..., 1], F32(0))
    r4 = np.where(inside, (R0[..., 2] + r[..., 2]) * half, R0[..., 2])
    r5 = np.where(inside, (R0[..., 3] + r[..., 3]) * half, R0[..., 3])
    r6 = np.where(inside, (R0[..., 4] + r[..., 4]) * quarter, R0[..., 4] * half)
    r2 = (R0[..., 0] - r2) * half
    r3 = (R0[..., 1] - r3) * half
    r2 = r2 + (r4 * dy + r6 * dx)
    r3 = r3 + (r6 * dy + r5 * dx)
    # OpenCV tests (unsigned)(x - 5) >= (unsigned)(w - 10) (and the same for y) before it scales; for
    # frames of 10 or more pixels that is "within 5 pixels of an edge"
    u = lambda v: np.asarray(v, np.int64) & 0xFFFFFFFF
    apply = (u(X - 5) >= u(w - 10)) | (u(Y - 5) >= u(h - 10))
    ones_x, ones_y = np.ones(w, F32), np.ones(h, F32)
    bx0 = np.where(np.arange(w) < 5, _BORDER[np.minimum(np.arange(w), 4)], ones_x)
    bx1 = np.where(np.arange(w) >= w - 5, _BORDER[np.clip(w - 1 - np.arange(w), 0, 4)], ones_x)
    by0 = np.where(np.arange(h) < 5, _BORDER[np.minimum(np.arange(h), 4)], ones_y)
    by1 = np.where(np.arange(h) >= h - 5, _BORDER[np.clip(h - 1 - np.arange(h), 0, 4)], ones_y)
    scale = ((bx0[None, :] * bx1[None, :]) * by0[:, None]) * by1[:, None]
    scale = np.where(apply, scale, one)
    r2, r3, r4, r5, r6 = (r * scale for r in (r2, r3, r4, r5, r6))
    return np.stack([r4 * r4 + r6 * r6, (r4 + r5) * r6, r5 * r5 + r6 * r6, r4 * r2 + r6 * r3, r6 * r2 + r5 * r3], -1)


# ---------------------------------------------------------------------------- step 7: UpdateFlow_Blur
def update_flow_blur(M, winsize):
    """FarnebackUpdateFlow_Blur's recurrences and solve: the new flow (h, w, 2) float32"""
    h, w = M.shape[:2]
    m = winsize // 2
    scale = 1.0 / (winsize * winsize)
    V = (M[0] * F32(m + 2)).astype(F64)
    for y in range(1, m):
        V = V + M[min(y, h - 1)].astype(F64)
    Vr = np.empty((h, w, 5), F64)
    for y in range(h):
        V = V + (M[min(y + m, h - 1)] - M[max(y - m - 1, 0)]).astype(F64)
        Vr[y] = V
    cx = lambda x: min(max(x, 0), w - 1)
    G = Vr[:, 0] * F64(m + 2)
    for x in range(1, m):
        G = G + Vr[:, cx(x)]
    flow = np.empty((h, w, 2), F32)
    for x in range(w):
        G = G + (Vr[:, cx(x + m)] - Vr[:, cx(x - m - 1)])
        g11, g12, g22, h1, h2 = (G[:, i] * scale for i in range(5))
        idet = 1.0 / (g11 * g22 - g12 * g12 + 1e-3)
        flow[:, x, 0] = ((g11 * h2 - g12 * h1) * idet).astype(F32)
        flow[:, x, 1] = ((g22 * h1 - g12 * h2) * idet).astype(F32)
    return flow


# ---------------------------------------------------------------------------- the whole call
def to_float32(frame):
    """convertTo(CV_32F)"""
    return np.ascontiguousarray(frame).astype(F32)


def farneback(prev, nxt, pyr_scale=0.5, levels=3, winsize=2, iterations=3, poly_n=5, poly_sigma=1.2, flags=0):
    """calcOpticalFlowFarneback(prev, next, None, ...) -> flow (h, w, 2) float32"""
    assert flags == 0 and poly_n in (5, 7)
    f = (to_float32(prev), to_float32(nxt))
    h, w = f[0].shape
    consts = poly_consts(poly_n, poly_sigma)
    flow = None
    for k, scale, sigma, ksize, lh, lw in level_plan(h, w, pyr_scale, levels):
        R0, R1 = (poly_exp(pyramid_image(fr, ksize, sigma, lh, lw), poly_n, consts) for fr in f)
        if flow is None:
            flow = np.zeros((lh, lw, 2), F32)
        else:
            flow = resize_linear(flow, lh, lw) * F32(1.0 / pyr_scale)
        M = update_matrices(R0, R1, flow)
        for it in range(iterations):
            flow = update_flow_blur(M, winsize)
            if it < iterations - 1:
                M = update_matrices(R0, R1, flow)
    return flow


def magnitude(flow):
    """cv2.cartToPolar(flow[..., 0], flow[..., 1])[0]"""
    fx, fy = flow[..., 0], flow[..., 1]
    return np.sqrt(fx * fx + fy * fy)


def optical_flow(frames, **params):
    """FilterOpticalFlow over a stack: (flow (n-1, h, w, 2), magnitude (n-1, h, w))"""
    flows = [farneback(frames[i], frames[i + 1], **params) for i in range(len(frames) - 1)]
    flows = np.stack(flows)
    return flows, magnitude(flows)


# ---------------------------------------------------------------------------- inputs
def hash_u32(idx, seed):
    """a fixed integer hash of uint32 indices (lowbias32), the same on every platform"""
    x = (np.asarray(idx, np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B9)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def texture_frames(n, h, w, seed, step=(1, 0), cell=8, noise=6):
    """n uint8 frames of a smooth texture (hash values on a coarse grid, bilinear in integers) moving by
    `step` whole pixels per frame, plus a little per-frame hash noise"""
    gh, gw = (h + 4 * n + 2 * cell) // cell + 2, (w + 4 * n + 2 * cell) // cell + 2
    grid = (hash_u32(np.arange(gh * gw), seed) % 200).astype(np.int64).reshape(gh, gw) + 20
    out = np.empty((n, h, w), np.uint8)
    for t in range(n):
        ys = np.arange(h)[:, None] - step[1] * t + 2 * n + cell
        xs = np.arange(w)[None, :] - step[0] * t + 2 * n + cell
        gy, fy = ys // cell, ys % cell
        gx, fx = xs // cell, xs % cell
        top = grid[gy, gx] * (cell - fx) + grid[gy, gx + 1] * fx
        bot = grid[gy + 1, gx] * (cell - fx) + grid[gy + 1, gx + 1] * fx
        v = (top * (cell - fy) + bot * fy) // (cell * cell)
        nz = hash_u32(np.arange(h * w) + t * h * w, seed + 7).reshape(h, w) % (2 * noise + 1)
        out[t] = np.clip(v + nz.astype(np.int64) - noise, 0, 255)
    return out


def smooth_texture(h, w, shift, seed=0):
    """float32 (h, w) of a smooth band-limited texture sampled at (x - dx, y - dy): for the accuracy check"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:h, :w].astype(F64)
    x, y = x - shift[0], y - shift[1]
    v = np.zeros((h, w))
    for _ in range(8):
        fx, fy = rng.uniform(-0.25, 0.25, 2)
        v += rng.uniform(10, 30) * np.cos(fx * x + fy * y + rng.uniform(0, 2 * np.pi))
    return (128 + v).astype(F32)


# ---------------------------------------------------------------------------- fixture
# (name, n, h, w, seed, step, dtype, params, full)
CASES = [
    ("ref_48x64", 3, 48, 64, 1, (1, 0), "u8", {}, True),
    ("ref_72x96", 2, 72, 96, 2, (2, 1), "u8", {}, True),
    ("p7_72x96", 2, 72, 96, 3, (0, 1), "u8", dict(poly_n=7, poly_sigma=1.5, winsize=5, iterations=2), True),
    ("w1_5x7", 2, 5, 7, 4, (1, 1), "u8", dict(winsize=1), True),
    ("f32_40x50", 2, 40, 50, 5, (1, 0), "f32", dict(pyr_scale=0.6, iterations=1), True),
    ("ref_240x320", 2, 240, 320, 6, (2, -1), "u8", {}, False),
]
POLY_CONSTS = [(5, 1.1), (5, 1.2), (7, 1.5)]
SAMPLE = 256


def case_frames(n, h, w, seed, step, dtype):
    fr = texture_frames(n, h, w, seed, step)
    if dtype == "f32":
        fr = fr.astype(F32) * F32(0.75) + F32(0.125)
    return fr


def params_of(extra):
    p = dict(REFERENCE_PARAMS)
    p.update(extra)
    return p


def sample_index(size, seed):
    return (hash_u32(np.arange(SAMPLE), seed + 99) % np.uint32(size)).astype(np.int64)


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def make():
    out = {}
    for n_, s in POLY_CONSTS:
        g, xg, xxg, ig = poly_consts(n_, s)
        key = "consts_%d_%g" % (n_, s)
        out[key + "_g"], out[key + "_xg"], out[key + "_xxg"] = g, xg, xxg
        out[key + "_ig"] = np.array(ig, F64)
    for name, n, h, w, seed, step, dtype, extra, full in CASES:
        fr = case_frames(n, h, w, seed, step, dtype)
        flow, mag = optical_flow(fr, **params_of(extra))
        if full:
            out[name + "_frames"] = fr
            out[name + "_flow"] = flow
            out[name + "_mag"] = mag
        else:
            out[name + "_frames_sha"] = sha(fr)
            out[name + "_flow_sha"] = sha(flow)
            out[name + "_mag_sha"] = sha(mag)
            idx = sample_index(mag.size, seed)
            out[name + "_mag_sample"] = mag.reshape(-1)[idx]
            out[name + "_flow_sample"] = flow.reshape(-1, 2)[idx]
    return out


if __name__ == "__main__":
    data = make()
    np.savez_compressed(OUT, **data)
    print("wrote %s (%d bytes, %d arrays)" % (OUT, os.path.getsize(OUT), len(data)))
