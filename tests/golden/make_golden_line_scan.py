#!/usr/bin/env python3
"""Generates tests/golden/line_scan_v1.npz -- line_scan, get_subimage and get_steepest_point
(video/analysis/image.py:61-127) as the reference's own code computes them over the NumPy restatement of the pinned
8-bit affine warp ("Affine warps and line scans").

    python tests/golden/make_golden_line_scan.py <reference checkout>      (or set $VA_REFERENCE)

Importing this module needs no checkout: the tests take the restatement (`get_affine_transform`, `invert`,
`warp_affine`, `line_scan`, `get_subimage`, and the 15-bit table form `warp_affine_table`), the case tables and the
seeded generators (`images`, `gpu_frames`, `gpu_batch`, `random_triples`) from it.  Writing the fixture lifts the
reference's line_scan, get_subimage and get_steepest_point with make_golden_polygon._lift at run time and runs them
in a namespace of shims; none of their source is stored.

Shims, and why none of them can change a result:
  cv2.getAffineTransform, cv2.warpAffine    `get_affine_transform` and `warp_affine` below (cv2 is not installed;
                                            both restate the classical fixed-point path of OpenCV 2.4 .. 4.10 as
                                            DESIGN.md §9 pins it -- agreement with a real cv2 is expected and
                                            unverified)
  round                                     Python 2's: halves away from zero (`py2_round`); the reference is
                                            Python 2 and get_subimage rounds its sizes with it
  ndimage.filters.gaussian_filter1d         scipy.ndimage.gaussian_filter1d, the same function under the name
                                            SciPy has since dropped
  `/`                                       true division: the reference has `from __future__ import division`,
                                            Python 3 needs none
Every case is compared exactly; none is dropped.
"""
import importlib.util
import math
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "line_scan_v1.npz")
EPS = 2.220446049250313e-16          # DBL_EPSILON
MAX_SIDE = 32767                     # VA_WARP_MAX_SIDE, include/videoanalysis_hip.h
COORD_LIMIT = float(1 << 30)         # VA_WARP_COORD_LIMIT: |fixed-point coordinate| of any destination pixel


def _sibling(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------- restatement
def py2_round(x):
    """Python 2's round(x): to the nearest integer, halves away from zero (a float)"""
    x = float(x)
    f = math.floor(abs(x))
    if abs(x) - f >= 0.5:
        f += 1.0
    return math.copysign(f, x)


def get_affine_transform(src, dst):
    """cv2.getAffineTransform: the 2x3 float64 matrix that maps three points onto three points.  Both triples are
    cast to float32 first; the 6x6 float64 system has rows i and i + 3 = (x_i, y_i, 1, 0, 0, 0 | X_i) and
    (0, 0, 0, x_i, y_i, 1 | Y_i); it is solved as cv::solve(DECOMP_LU) does, operation by operation.  A pivot below
    100 eps raises ValueError."""
    src = np.asarray(src, np.float32).reshape(3, 2)
    dst = np.asarray(dst, np.float32).reshape(3, 2)
    a = [[0.0] * 6 for _ in range(6)]
    b = [0.0] * 6
    for i in range(3):
        x, y = float(src[i, 0]), float(src[i, 1])
        a[i][0], a[i][1], a[i][2] = x, y, 1.0
        a[i + 3][3], a[i + 3][4], a[i + 3][5] = x, y, 1.0
        b[i], b[i + 3] = float(dst[i, 0]), float(dst[i, 1])
    for i in range(6):
        k = i
        for j in range(i + 1, 6):
            if abs(a[j][i]) > abs(a[k][i]):
                k = j
        if abs(a[k][i]) < EPS * 100:
            raise ValueError("get_affine_transform: the three source points are collinear")
        if k != i:
            a[i], a[k] = a[k], a[i]
            b[i], b[k] = b[k], b[i]
        d = -1 / a[i][i]
        for j in range(i + 1, 6):
            alpha = a[j][i] * d
            for c in range(i + 1, 6):
                a[j][c] += alpha * a[i][c]
            b[j] += alpha * b[i]
    for i in range(5, -1, -1):
        s = b[i]
        for c in range(i + 1, 6):
            s -= a[i][c] * b[c]
        b[i] = s / a[i][i]
    return np.array(b, np.float64).reshape(2, 3)


def invert(M):
    """the inverse map of cv::warpAffine, in its float64 operation order"""
    m0, m1, m2, m3, m4, m5 = (float(v) for v in np.asarray(M, np.float64).reshape(6))
    D = m0 * m4 - m1 * m3
    D = 1 / D if D != 0 else 0.0
    A11, A22 = m4 * D, m0 * D
    m0 = A11
    m1 *= -D
    m3 *= -D
    m4 = A22
    b1 = -m0 * m2 - m1 * m5
    b2 = -m3 * m2 - m4 * m5
    return np.array([[m0, m1, b1], [m3, m4, b2]], np.float64)


def within_limits(Minv, dw, dh):
    """what the kernels take: sides 0 .. MAX_SIDE and every fixed-point coordinate below COORD_LIMIT in magnitude
    (bounded by the sum of the magnitudes of its terms, so a NaN or an infinity fails too)"""
    if not (0 <= dw <= MAX_SIDE and 0 <= dh <= MAX_SIDE):
        return False
    m = np.asarray(Minv, np.float64).reshape(6)
    xs, ys = float(max(dw - 1, 0)), float(max(dh - 1, 0))
    bx = (abs(m[0]) * xs + abs(m[1]) * ys + abs(m[2])) * 1024
    by = (abs(m[3]) * xs + abs(m[4]) * ys + abs(m[5])) * 1024
    return bool(bx < COORD_LIMIT and by < COORD_LIMIT)


def _coordinates(Minv, dw, dh):
    """(X, Y) int64 (dh, dw): the source coordinates of every destination pixel in 1/32 px"""
    m = np.asarray(Minv, np.float64).reshape(6)
    x = np.arange(dw, dtype=np.float64)
    y = np.arange(dh, dtype=np.float64)
    adelta = np.rint(m[0] * x * 1024).astype(np.int64)
    bdelta = np.rint(m[3] * x * 1024).astype(np.int64)
    X0 = np.rint((m[1] * y + m[2]) * 1024).astype(np.int64) + 16
    Y0 = np.rint((m[4] * y + m[5]) * 1024).astype(np.int64) + 16
    return (X0[:, None] + adelta[None, :]) >> 5, (Y0[:, None] + bdelta[None, :]) >> 5


def _taps(img, X, Y):
    h, w = img.shape
    sx, sy = X >> 5, Y >> 5

    def at(yy, xx):
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        return np.where(ok, img[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], 0).astype(np.int64)
    return at(sy, sx), at(sy, sx + 1), at(sy + 1, sx), at(sy + 1, sx + 1), X & 31, Y & 31


def warp_affine(img, M, dsize, inverse=False):
    """cv2.warpAffine(img, M, dsize) of a 2-d uint8 image with INTER_LINEAR and BORDER_CONSTANT 0; dsize = (width,
    height) as cv2 takes it; inverse: the WARP_INVERSE_MAP flag (M maps destination to source as it is)"""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 2:
        raise TypeError("warp_affine: 2-d uint8 images only")
    dw, dh = int(dsize[0]), int(dsize[1])
    Minv = np.asarray(M, np.float64).reshape(2, 3) if inverse else invert(M)
    if not within_limits(Minv, dw, dh):
        raise ValueError("warp_affine: beyond the limits (sides up to %d, coordinates below 2^20 px)" % MAX_SIDE)
    X, Y = _coordinates(Minv, dw, dh)
    v00, v01, v10, v11, fx, fy = _taps(img, X, Y)
    out = ((32 - fx) * (32 - fy) * v00 + fx * (32 - fy) * v01 + (32 - fx) * fy * v10 + fx * fy * v11 + 512) >> 10
    return out.astype(np.uint8)


def bilinear_table(spill=1):
    """OpenCV's 15-bit weight table of INTER_LINEAR for 8-bit remaps, (32, 32, 4) int64 indexed [fy, fx]: the float
    weights times 32768 as shorts.  Every product is an exact integer below 32768 except the 32768 of fx = fy = 0,
    which saturates to 32767; the table's sum correction then puts the missing 1 on another tap (`spill`: which)."""
    f = np.arange(32, dtype=np.float32) / np.float32(32)
    wy = np.stack([1 - f, f], 1)
    tab = np.zeros((32, 32, 4), np.int64)
    for iy in range(32):
        for ix in range(32):
            w4 = np.array([wy[iy, 0] * wy[ix, 0], wy[iy, 0] * wy[ix, 1], wy[iy, 1] * wy[ix, 0],
                           wy[iy, 1] * wy[ix, 1]], np.float32) * np.float32(32768)
            q = np.clip(np.rint(w4.astype(np.float64)), -32768, 32767).astype(np.int64)
            if q.sum() != 32768:
                q[spill] += 32768 - q.sum()
            tab[iy, ix] = q
    return tab


def warp_affine_table(img, M, dsize, inverse=False, spill=1):
    """warp_affine through the 15-bit table: (sum of weight * tap + 2^14) >> 15"""
    img = np.asarray(img)
    dw, dh = int(dsize[0]), int(dsize[1])
    Minv = np.asarray(M, np.float64).reshape(2, 3) if inverse else invert(M)
    X, Y = _coordinates(Minv, dw, dh)
    v00, v01, v10, v11, fx, fy = _taps(img, X, Y)
    t = bilinear_table(spill)[fy, fx]
    out = (t[..., 0] * v00 + t[..., 1] * v01 + t[..., 2] * v10 + t[..., 3] * v11 + (1 << 14)) >> 15
    return out.astype(np.uint8)


def scan_geometry(p1, p2, half_width):
    """(source triple, destination triple, rows, cols) of line_scan, the reference's float64 arithmetic"""
    length = np.hypot(p2[0] - p1[0], p2[1] - p1[1])
    angle = np.arctan2(p2[1] - p1[1], p2[0] - p1[0])
    p0 = (p1[0] + half_width * np.sin(angle), p1[1] - half_width * np.cos(angle))
    src = np.array((p0, (p1[0], p1[1]), (p2[0], p2[1])), np.float32)
    dst = np.array(((0, 0), (0, half_width), (length, half_width)), np.float32)
    return src, dst, int(2 * half_width), int(length)


def line_scan_strip(img, p1, p2, half_width=5):
    """(matrix, strip) of line_scan; an empty strip raises ValueError (the documented deviation)"""
    src, dst, rows, cols = scan_geometry(p1, p2, half_width)
    if rows < 1 or cols < 1:
        raise ValueError("line_scan: empty strip (%d rows, %d columns)" % (rows, cols))
    M = get_affine_transform(src, dst)
    return M, warp_affine(img, M, (cols, rows))


def line_scan(img, p1, p2, half_width=5):
    strip = line_scan_strip(img, p1, p2, half_width)[1]
    return strip.sum(axis=0, dtype=np.int64).astype(np.float64) / strip.shape[0]


def subimage_geometry(slice_x, slice_y, width=None, height=None):
    """(source triple, destination triple, (dw, dh)) of get_subimage, its transposed naming included"""
    p1_x, p2_x = slice_x[:2]
    p1_y, p2_y = slice_y[:2]
    if width is None:
        width = p2_x - p1_x
    if height is None:
        height = (p2_y - p1_y) * width / (p2_x - p1_x)
    src = np.array(((p1_x, p1_y), (p1_x, p2_y), (p2_x, p1_y)), np.float32)
    dst = np.array(((0, 0), (height, 0), (0, width)), np.float32)
    return src, dst, (int(py2_round(height)), int(py2_round(width)))


def get_subimage(img, slice_x, slice_y, width=None, height=None):
    src, dst, dsize = subimage_geometry(slice_x, slice_y, width, height)
    if dsize[0] < 1 or dsize[1] < 1:
        raise ValueError("get_subimage: empty destination %r" % (dsize,))
    return warp_affine(img, get_affine_transform(src, dst), dsize)


# --------------------------------------------------------------------------------------- generators
def images():
    """name -> uint8 image of the fixture"""
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[:60, :80]
    ramp = (2 * xx + 3 * yy + 40 * np.sin(xx / 7.0) * np.cos(yy / 5.0)) % 256
    return {"noise": rng.integers(0, 256, (60, 80), dtype=np.uint8), "ramp": ramp.astype(np.uint8),
            "odd": rng.integers(0, 256, (47, 61), dtype=np.uint8), "white": np.full((33, 45), 255, np.uint8)}


# (image, p1, p2, half width) of the fixture's scans
SCAN_CASES = [
    ("noise", (10, 30), (50, 30), 3), ("noise", (10, 30), (10, 5), 2), ("noise", (50, 30), (10, 30), 3),
    ("noise", (10, 5), (10, 30), 2), ("noise", (5.5, 7.25), (70.1, 50.9), 5), ("noise", (70, 50), (6, 8), 5),
    ("noise", (-10, 20), (30, 25), 4), ("noise", (60, 40), (95, 70), 2.5), ("noise", (20, -8), (25, 30), 1),
    ("noise", (30, 50), (28, 75), 7), ("noise", (0, 59), (79, 59), 1), ("noise", (79, 0), (79, 59), 1),
    ("noise", (12.3, 40.7), (13.4, 40.9), 0.5), ("noise", (3, 3), (5.2, 3), 1.5),
    ("ramp", (10, 30), (50, 30), 3), ("ramp", (8.2, 11.9), (66.6, 44.4), 5), ("ramp", (40, 55), (41, 2), 6),
    ("ramp", (75, 30), (2, 29), 0.5), ("ramp", (-20, -20), (100, 80), 5), ("ramp", (200, 200), (260, 220), 5),
    ("odd", (0, 0), (60, 46), 5), ("odd", (60, 0), (0, 46), 2.5), ("odd", (30.5, 23.5), (31.5, 23.5), 7),
    ("odd", (-5, 46), (70, 46), 1), ("odd", (60, -5), (60, 55), 1), ("odd", (2, 40), (58, 4), 3.7),
    ("white", (-4, 10), (50, 10), 3), ("white", (5, 5), (40, 28), 5), ("white", (22, -6), (22, 40), 2),
    ("white", (10.5, 10.5), (30.5, 20.5), 2.5),
]

# (image, slice_x, slice_y, width, height) of the fixture's sub-images
SUBIMAGE_CASES = [
    ("noise", (10, 50), (5, 35), None, None), ("noise", (10, 50), (5, 35), 20, None), ("noise", (10, 50), (5, 35), 20, 30),
    ("noise", (10.5, 30.25), (7.75, 20.5), None, None), ("noise", (0, 80), (0, 60), 33, None),
    ("noise", (-5, 20), (-5, 20), 12.5, 12.5), ("noise", (60, 100), (40, 80), 17, 9), ("ramp", (20, 41), (10, 24), 10.5, None),
    ("ramp", (50, 10), (5, 35), 40, 30), ("ramp", (5, 6), (5, 6), 1, 1), ("odd", (0, 61), (0, 47), None, None),
    ("white", (-3, 48), (-3, 36), 25, 19), ("odd", (3, 60), (2, 45), 7.5, 6.5),
]

# (profile name, direction, smoothing) of the fixture's steepest points
STEEPEST_CASES = [("step", 1, 0), ("step", -1, 0), ("step", 1, 2), ("step", -1, 1.5), ("noisy", 1, 0), ("noisy", -1, 0),
                  ("noisy", 1, 3), ("noisy", -1, 0.7), ("flat", 1, 0), ("flat", -1, 2), ("two", 1, 0), ("two", -1, 1),
                  ("one", 1, 0), ("empty", 1, 0), ("scan", 1, 0), ("scan", -1, 2)]


def profiles():
    rng = np.random.default_rng(9)
    x = np.arange(64, dtype=np.float64)
    step = 20 + 100 / (1 + np.exp(-(x - 37.3) / 2.0)) - 60 / (1 + np.exp(-(x - 12.1) / 1.5))
    return {"step": step, "noisy": step + rng.normal(0, 6, 64), "flat": np.full(9, 3.0), "two": np.array([1.0, 4.0]),
            "one": np.array([2.0]), "empty": np.zeros(0),
            "scan": line_scan(images()["ramp"], (8.2, 11.9), (66.6, 44.4), 5)}


def gpu_frames():
    """the 3 frames of 47 x 61 of the GPU test; the last is uniform 255"""
    f = np.random.default_rng(11).integers(0, 256, (3, 47, 61), dtype=np.uint8)
    f[2] = 255
    return f


GPU_LENGTHS = (1, 2, 63, 64, 65, 128, 129)
GPU_HALF_WIDTHS = (0.5, 1, 2.5, 5, 7)


def gpu_batch():
    """the ragged batch of the GPU test: (frame, p1, p2, half width), about 400 scans over gpu_frames()"""
    rng = np.random.default_rng(12)
    out = []
    for k, L in enumerate(GPU_LENGTHS):                      # every length with every half width, exact and slanted
        for j, hw in enumerate(GPU_HALF_WIDTHS):
            x0 = -3.0 if L > 2 else 5.0
            out.append(((k + j) % 3, (x0, 20.0 + j), (x0 + L, 20.0 + j), hw))
            a = 0.3 + 0.9 * j + 0.2 * k
            out.append(((k + j + 1) % 3, (30.25, 21.5), (30.25 + (L + 0.5) * math.cos(a), 21.5 + (L + 0.5) * math.sin(a)), hw))
    for f in range(3):                                       # the four axis directions at integer coordinates
        out += [(f, (10, 30), (50, 30), 3), (f, (50, 30), (10, 30), 3), (f, (10, 5), (10, 40), 2), (f, (10, 40), (10, 5), 2)]
    out += [(0, (20, 46), (60, 46), 1), (0, (60, 5), (60, 46), 1), (1, (0, 46), (60, 46), 2), (1, (60, 0), (60, 46), 2),
            (0, (60, 46), (20, 46), 1), (0, (60, 46), (60, 5), 1)]          # ending on the last row and column
    out += [(0, (-10, 20), (20, 22), 2.5), (1, (50, 20), (75, 25), 5), (0, (30, -9), (33, 15), 2.5),
            (1, (30, 35), (28, 60), 5), (2, (-10, 20), (20, 22), 2.5), (2, (50, 20), (75, 25), 5),
            (2, (30, -9), (33, 15), 2.5), (2, (30, 35), (28, 60), 5)]       # crossing each of the four borders
    out += [(0, (-20.5, -7.25), (-2.5, -1.5), 5), (1, (-30, 10), (-4, -12), 2.5), (0, (-6, -6), (8, 9), 7)]   # negative
    out += [(0, (100, 100), (150, 120), 5), (2, (-80, -80), (-20, -60), 5)]                                # outside
    while len(out) < 400:
        p1 = (float(rng.uniform(-12, 72)), float(rng.uniform(-10, 56)))
        p2 = (float(rng.uniform(-12, 72)), float(rng.uniform(-10, 56)))
        if math.hypot(p2[0] - p1[0], p2[1] - p1[1]) < 1:
            continue
        if rng.random() < 0.3:                               # integer end points: exact grid hits, fx = fy = 0 taps
            p1, p2 = (float(round(p1[0])), float(round(p1[1]))), (float(round(p2[0])), float(round(p2[1])))
            if p1 == p2:
                continue
        out.append((int(rng.integers(0, 3)), p1, p2, float(rng.choice(GPU_HALF_WIDTHS))))
    return out


def random_triples(seed, count):
    """(src, dst) float64 (count, 3, 2): seeded point triples, a share of them line_scan and get_subimage shaped"""
    rng = np.random.default_rng(seed)
    src = rng.uniform(-50, 500, (count, 3, 2))
    dst = rng.uniform(-50, 500, (count, 3, 2))
    for k in range(0, count, 3):
        s, d, _, _ = scan_geometry(tuple(rng.uniform(-20, 300, 2)), tuple(rng.uniform(-20, 300, 2)),
                                   float(rng.choice(GPU_HALF_WIDTHS)))
        src[k], dst[k] = s, d
    for k in range(1, count, 7):
        a, b = np.sort(rng.integers(0, 300, 2)), np.sort(rng.integers(0, 300, 2))
        s, d, _ = subimage_geometry((int(a[0]), int(a[1]) + 1), (int(b[0]), int(b[1]) + 1), float(rng.integers(1, 90)))
        src[k], dst[k] = s, d
    return src, dst


# -------------------------------------------------------------------------------------------- lifting
SHIMS = ["cv2.getAffineTransform -> get_affine_transform (the restatement)",
         "cv2.warpAffine -> warp_affine (the restatement)",
         "round -> Python 2's, halves away from zero",
         "ndimage.filters.gaussian_filter1d -> scipy.ndimage.gaussian_filter1d",
         "division -> Python 3's true division (the reference imports it from __future__)"]


def load_reference(root):
    """(line_scan, get_subimage, get_steepest_point) of the reference, lifted and shimmed"""
    from scipy import ndimage
    POL = _sibling("make_golden_polygon")
    cv2 = types.ModuleType("cv2_shim")
    cv2.getAffineTransform = get_affine_transform
    cv2.warpAffine = lambda img, matrix, dsize: warp_affine(img, matrix, dsize)
    nd = types.ModuleType("ndimage_shim")
    nd.filters = types.ModuleType("ndimage_filters_shim")
    nd.filters.gaussian_filter1d = ndimage.gaussian_filter1d
    ns = {"np": np, "cv2": cv2, "round": py2_round, "ndimage": nd, "__name__": "ref_image"}
    POL._lift(os.path.join(root, "video", "analysis", "image.py"), ("line_scan", "get_subimage", "get_steepest_point"),
              ns)
    return ns["line_scan"], ns["get_subimage"], ns["get_steepest_point"]


def generate(root):
    ref_scan, ref_sub, ref_steep = load_reference(root)
    imgs = images()
    data = {"shims": np.array(SHIMS)}
    for name, img in imgs.items():
        data["image/%s" % name] = img
    for k, (name, p1, p2, hw) in enumerate(SCAN_CASES):
        M, strip = line_scan_strip(imgs[name], p1, p2, hw)
        ref = ref_scan(imgs[name], p1, p2, hw)
        assert ref.dtype == np.float64 and np.array_equal(ref, line_scan(imgs[name], p1, p2, hw)), k
        assert np.array_equal(ref, strip.mean(axis=0)), k
        data["scan/%d/points" % k] = np.array([p1, p2], np.float64)
        data["scan/%d/half_width" % k] = np.float64(hw)
        data["scan/%d/matrix" % k] = M
        data["scan/%d/strip" % k] = strip
        data["scan/%d/profile" % k] = ref
    for k, (name, sx, sy, width, height) in enumerate(SUBIMAGE_CASES):
        ref = ref_sub(imgs[name], sx, sy, width, height)
        assert ref.dtype == np.uint8 and np.array_equal(ref, get_subimage(imgs[name], sx, sy, width, height)), k
        src, dst, dsize = subimage_geometry(sx, sy, width, height)
        assert ref.shape == (dsize[1], dsize[0]), k
        data["sub/%d/matrix" % k] = get_affine_transform(src, dst)
        data["sub/%d/image" % k] = ref
    prof = profiles()
    for name, p in prof.items():
        data["profile/%s" % name] = p
    for k, (name, direction, smoothing) in enumerate(STEEPEST_CASES):
        data["steepest/%d" % k] = np.float64(ref_steep(prof[name], direction, smoothing))
    return data


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("VA_REFERENCE")
    if not root or not os.path.isdir(os.path.join(root, "video", "analysis")):
        sys.stderr.write("usage: make_golden_line_scan.py <reference checkout> (or $VA_REFERENCE); nothing written\n")
        raise SystemExit(2)
    data = generate(root)
    np.savez_compressed(OUT, **data)
    print("wrote %s (%d arrays, %d bytes)" % (OUT, len(data), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
