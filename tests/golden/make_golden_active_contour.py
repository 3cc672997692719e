#!/usr/bin/env python3
"""Generates tests/golden/active_contour_v1.npz -- ActiveContour (video/analysis/active_contour.py) as the
reference's own code computes it, and the NumPy restatement of the GPU path's pinned arithmetic.

    python tests/golden/make_golden_active_contour.py <reference checkout>      (or set $VA_REFERENCE)

Importing this module needs no checkout: the tests take the restatement (`sobel5`, `gradients`, `snake`,
`fixed_sum`) and the case tables from it.  Writing the fixture lifts ActiveContour and the curve and image
helpers out of the checkout with `ast` at run time and runs them in a namespace of shims; none of their
source is stored.

Shims, and why none of them can change a result:
  xrange -> range, itertools.izip -> zip   the Python 3 names of the same iterations
  np.int -> np.int64                       NumPy 2 removed the alias of the platform integer (int64 here)
  DictFiniteCapacity -> dict               a cache of matrices computed from their key; it only saves time
  cv2.arcLength -> curve_length below      OpenCV's open-curve arcLength restated: float32 dx*dx + dy*dy,
                                           float32 sqrt, summed in double in point order (cv2 is not
                                           installed; the restatement is the one video.analysis.curves uses)
  fx, fy set from `gradients` below        set_potential is bypassed: its cv2.GaussianBlur is the oracle's
                                           gaussian_f32 / gaussian_u8 (the definitions the GPU blur is pinned
                                           to) and its two cv2.Sobel calls are `sobel5` below

Sobel: OpenCV's FilterEngine with a CV_64F kernel -- row pass s = k0*S[x-2], s += k_i*S[x-2+i]
for i = 1..4 (the zero tap included); column pass symmetric s = 6*S[y] + 0.0, s += 4*(S[y+1] + S[y-1]),
s += 1*(S[y+2] + S[y-2]), antisymmetric s = 0.0, s += 2*(S[y+1] - S[y-1]), s += 1*(S[y+2] - S[y-2]);
fx = column-smooth(row-derivative), fy = column-derivative(row-smooth); BORDER_REFLECT_101.

Snake: the reference's loop with the matrix-vector product summed in ascending column order (its np.dot goes
through BLAS in an order of its own) and the residual / total variation summed by `fixed_sum`, the kernel's
order.  Each snake case keeps the smallest relative margin |residual - tol*gamma| / (tol*gamma) over its
iterations (from the restatement, which follows the reference to ~1e-11 px); only cases with a margin of at
least MIN_MARGIN are kept, so that a last-bit difference in the residual cannot change an iteration count.
"""
import ast
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "active_contour_v1.npz")
MIN_MARGIN = 1e-6

SHIMS = ("xrange -> range", "itertools.izip -> zip", "np.int -> np.int64", "DictFiniteCapacity -> dict",
         "cv2.arcLength -> float32 restatement", "fx, fy <- oracle blur + restated Sobel (set_potential bypassed)")

# (h, w) of the Sobel cases, on uint8 and float32 inputs
SOBEL_SIZES = ((1, 1), (1, 7), (2, 2), (3, 5), (5, 5), (6, 9), (37, 53))
# blur + Sobel at 48 x 64
BLUR_SIGMAS = (1.0, 2.5, 10.0)
BIG = (1080, 1920, 10.0)             # float32, sigma = 10: sha256 + strided sample
SAMPLE_STRIDE = 997

PARAMS = {"ref": dict(blur_radius=10, alpha=0.0, beta=1e2, gamma=0.001),
          "centre": dict(blur_radius=1, alpha=1e3, beta=1e6, gamma=0.01)}
POT_SHAPE = (120, 160)


# ---------------------------------------------------------------------------------------- inputs
def ramp(shape, salt=0):
    """a deterministic image with fine structure: ((i * 2654435761) >> 13) & 255 over the flat index"""
    i = np.arange(int(np.prod(shape)), dtype=np.uint64) + np.uint64(salt)
    return (((i * np.uint64(2654435761)) >> np.uint64(13)) & np.uint64(255)).astype(np.uint8).reshape(shape)


def sobel_input(h, w, dtype, salt=0):
    v = ramp((h, w), salt)
    if dtype == np.uint8:
        return v
    # negatives, zeros (for the sign of zero results) and non-trivial mantissas
    f = (v.astype(np.float32) - 128.0) * np.float32(0.37)
    f[::3, ::2] = 0.0
    return f.astype(np.float32)


def potential(kind):
    """the snake cases' potentials: a ridge along an ellipse (the snake climbs the gradient, as onto the
    ridge of a distance transform) plus ripples, float32 or uint8 ("f32", "u8"); the "_soft" kinds have a
    lower, wider ridge for the centre-line parameters, whose gamma = 0.01 makes the steep one chaotic (the
    last-bit differences of the matrix product grow to pixels within 1000 iterations)"""
    h, w = POT_SHAPE
    y, x = np.mgrid[:h, :w].astype(np.float64)
    r = np.sqrt(((x - 80.0) / 52.0) ** 2 + ((y - 60.0) / 38.0) ** 2)
    height, width = (20.0, 0.5) if kind.endswith("_soft") else (200.0, 0.25)
    p = height * np.exp(-((r - 1.0) / width) ** 2) + 3.0 * np.sin(x / 5.0) * np.cos(y / 7.0) + 20.0
    if kind.startswith("u8"):
        return np.clip(np.round(p), 0, 255).astype(np.uint8)
    return p.astype(np.float32)


def ellipse_curve(N, closed, scale=1.15, shift=(0.0, 0.0), phase=0.3):
    """N points on an ellipse around the potential's valley (an arc of 300 degrees when open)"""
    span = 2 * np.pi * (1 - 1.0 / N) if closed else 2 * np.pi * 300 / 360
    t = phase + np.linspace(0, span, N)
    x = 80.0 + scale * 52.0 * np.cos(t) + shift[0]
    y = 60.0 + scale * 38.0 * np.sin(t) + shift[1]
    return np.stack([x, y], axis=1)


def clustered_curve(N):
    """an open curve whose first points crowd together, so that several anchors pick one equidistant point"""
    t = np.concatenate([np.linspace(0, 0.02, 6), np.linspace(0.05, 1, N - 6)])
    return np.stack([30.0 + 100.0 * t, 50.0 + 25.0 * np.sin(3 * t)], axis=1)


# (name, potential kind, params, closed, N, max_iterations, anchor_x, anchor_y, curve kind)
# anchors: None, an index list or ("mask", indices) for a boolean mask of the curve's points
SNAKE_CASES = [
    ("open_ref_n64_it50", "f32", "ref", False, 64, 50, None, None, "ellipse"),
    ("closed_ref_n64_it50", "f32", "ref", True, 64, 50, None, None, "ellipse"),
    ("closed_ref_n128_it50", "u8", "ref", True, 128, 50, None, None, "ellipse"),
    ("open_centre_n64_it1000", "f32_soft", "centre", False, 64, 1000, None, None, "ellipse"),
    ("closed_centre_n200_it1000", "u8_soft", "centre", True, 200, 1000, None, None, "ellipse"),
    ("open_centre_n64_it1", "f32_soft", "centre", False, 64, 1, None, None, "ellipse"),
    ("closed_ref_n64_it1", "u8", "ref", True, 64, 1, None, None, "ellipse"),
    ("open_ref_n3_it50", "f32", "ref", False, 3, 50, None, None, "ellipse"),
    ("open_ref_n4_it50", "f32", "ref", False, 4, 50, None, None, "ellipse"),
    ("closed_ref_n5_it50", "f32", "ref", True, 5, 50, None, None, "ellipse"),
    ("closed_centre_n5_it1000", "f32_soft", "centre", True, 5, 1000, None, None, "ellipse"),
    ("open_ref_n600_it50", "f32", "ref", False, 600, 50, None, None, "ellipse"),
    ("closed_ref_n600_it50", "u8", "ref", True, 600, 50, None, None, "ellipse"),
    ("open_centre_anchor_xy_idx", "f32_soft", "centre", False, 64, 1000, [0, 63], [0, 63], "ellipse"),
    ("open_centre_anchor_x_only", "f32_soft", "centre", False, 64, 1000, [0, 20, 63], None, "ellipse"),
    ("open_ref_anchor_y_mask", "f32", "ref", False, 64, 50, None, ("mask", [0, 10, 40]), "ellipse"),
    ("open_centre_anchor_dups", "u8_soft", "centre", False, 40, 1000, [0, 1, 2, 3, 2, 39], [5, 4, 0, 1], "clustered"),
    ("closed_ref_outside", "f32", "ref", True, 64, 50, None, None, "outside"),
    ("open_centre_outside_anchor", "u8_soft", "centre", False, 64, 1000, [0], [63], "outside"),
    ("closed_ref_tol1500", "f32", "ref", True, 64, 1000, None, None, "ellipse"),
    ("open_ref_tol3000", "u8", "ref", False, 64, 1000, None, None, "ellipse"),
    ("closed_ref_n200_tol3000", "u8", "ref", True, 200, 1000, None, None, "ellipse"),
    ("open_ref_anchor_tol3000", "f32", "ref", False, 64, 1000, [0], [0, 63], "ellipse"),
    ("open_ref_n2", "f32", "ref", False, 2, 50, None, None, "ellipse"),
    ("open_ref_n1", "f32", "ref", False, 1, 50, None, None, "ellipse"),
]


# residual_tolerance of the cases that are to stop before max_iterations (the class default, 1, elsewhere)
TOLERANCE = {"closed_ref_tol1500": 1500, "open_ref_tol3000": 3000, "closed_ref_n200_tol3000": 3000,
             "open_ref_anchor_tol3000": 3000}


def case_curve(N, closed, kind):
    if kind == "clustered":
        return clustered_curve(N)
    if kind == "outside":        # partly beyond the left and the bottom edge: clipped before the first step
        return ellipse_curve(N, closed, scale=1.6, shift=(-20.0, 14.0))
    return ellipse_curve(N, closed)


def case_anchor(spec, N):
    if spec is None:
        return None
    if isinstance(spec, tuple) and spec[0] == "mask":
        m = np.zeros(N, bool)
        m[list(spec[1])] = True
        return m
    return list(spec)


# ---------------------------------------------------------------------------------- restatement
def reflect101(idx, n):
    idx = np.asarray(idx).copy()
    if n == 1:
        return np.zeros_like(idx)
    while True:
        lo, hi = idx < 0, idx >= n
        if not (lo.any() or hi.any()):
            return idx
        idx = np.where(lo, -idx, np.where(hi, 2 * (n - 1) - idx, idx))


def sobel5(frames):
    """(fx, fy) float64 of uint8 / float32 (h, w) or (n, h, w) frames: cv2.Sobel(p, CV_64F, 1, 0, 5) and
    (0, 1, 5) in FilterEngine's order"""
    a = np.asarray(frames)
    single = a.ndim == 2
    S = (a[None] if single else a).astype(np.float64)
    n, h, w = S.shape
    R = S[:, :, reflect101(np.arange(-2, w + 2), w)]
    t = [R[:, :, i:i + w] for i in range(5)]
    d = -1.0 * t[0]
    d = d + -2.0 * t[1]
    d = d + 0.0 * t[2]
    d = d + 2.0 * t[3]
    d = d + 1.0 * t[4]
    s = 1.0 * t[0]
    s = s + 4.0 * t[1]
    s = s + 6.0 * t[2]
    s = s + 4.0 * t[3]
    s = s + 1.0 * t[4]
    rows = reflect101(np.arange(-2, h + 2), h)
    u = [d[:, rows][:, i:i + h] for i in range(5)]
    v = [s[:, rows][:, i:i + h] for i in range(5)]
    fx = 6.0 * u[2] + 0.0
    fx = fx + 4.0 * (u[3] + u[1])
    fx = fx + 1.0 * (u[4] + u[0])
    fy = 0.0 + 2.0 * (v[3] - v[1])
    fy = fy + 1.0 * (v[4] - v[0])
    return (fx[0], fy[0]) if single else (fx, fy)


def blur(frames, sigma):
    """cv2.GaussianBlur(p, (0, 0), sigma) as the oracle defines it (the GPU's va_gaussian_u8 / _f32)"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import oracle as O
    a = np.asarray(frames)
    return O.gaussian_u8(a, sigma) if a.dtype == np.uint8 else O.gaussian_f32(a, sigma)


def gradients(p, blur_radius):
    """set_potential: blur when blur_radius > 0, then both Sobel planes"""
    return sobel5(blur(p, blur_radius) if blur_radius > 0 else p)


def fixed_sum(e):
    """the kernel's reduction of the terms e (x terms of every point, then y terms): thread t adds
    e[t], e[t + 256], ... starting from 0.0, then the 256 partials are folded in halves"""
    k = max(1, -(-len(e) // 256))
    a = np.zeros(k * 256)
    a[:len(e)] = e
    acc = np.zeros(256)
    for row in a.reshape(k, 256):
        acc = acc + row
    while len(acc) > 1:
        half = len(acc) // 2
        acc = acc[:half] + acc[half:]
    return float(acc[0])


def subpixels(img, pts):
    """image.subpixels"""
    x, y = pts[:, 0], pts[:, 1]
    xi = x.astype(np.int64)
    yi = y.astype(np.int64)
    dx = x - xi
    dy = y - yi
    return ((1.0 - dx) * (1.0 - dy) * img[yi, xi] + dx * (1.0 - dy) * img[yi, xi + 1] +
            (1.0 - dx) * dy * img[yi + 1, xi] + dx * dy * img[yi + 1, xi + 1])


def matvec(P, r):
    """P @ r with acc = P[i, 0]*r[0], acc += P[i, j]*r[j] for ascending j"""
    acc = P[:, 0] * r[0]
    for j in range(1, len(r)):
        acc = acc + P[:, j] * r[j]
    return acc


def snake(fx, fy, points, Pinv, gamma, tol_gamma, max_iterations, flags=None, vals=None):
    """the snake kernel's loop on one contour; returns (points, iterations, total_variation, margin)"""
    h, w = fx.shape
    p = np.array(points, np.float64)
    p[:, 0] = np.clip(p[:, 0], 0, w - 2)
    p[:, 1] = np.clip(p[:, 1], 0, h - 2)
    start = p.copy()
    margin = np.inf
    k = 0
    for k in range(max_iterations):
        rx = p[:, 0] + gamma * subpixels(fx, p)
        ry = p[:, 1] + gamma * subpixels(fy, p)
        qx, qy = matvec(Pinv, rx), matvec(Pinv, ry)
        if flags is not None:
            qx = np.where(flags & 1, vals[:, 0], qx)
            qy = np.where(flags & 2, vals[:, 1], qy)
        residual = fixed_sum(np.concatenate([np.abs(qx - p[:, 0]), np.abs(qy - p[:, 1])]))
        p = np.stack([np.clip(qx, 0, w - 2), np.clip(qy, 0, h - 2)], axis=1)
        if tol_gamma > 0:
            margin = min(margin, abs(residual - tol_gamma) / tol_gamma)
        if residual < tol_gamma:
            break
    tv = fixed_sum(np.concatenate([np.abs(start[:, 0] - p[:, 0]), np.abs(start[:, 1] - p[:, 1])]))
    return p, k + 1, tv, margin


def sha(a):
    a = np.ascontiguousarray(a)
    return np.array(hashlib.sha256(a.dtype.str.encode() + str(a.shape).encode() + a.tobytes()).hexdigest())


# ---------------------------------------------------------------------------------------- lifting
def _lift(path, names, ns):
    tree = ast.parse(open(path).read(), path)
    keep, found = [], set()
    for node in tree.body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)) and node.name in names:
            keep.append(node)
            found.add(node.name)
    missing = set(names) - found
    if missing:
        raise SystemExit("%s: not found in the checkout: %s" % (path, sorted(missing)))
    mod = ast.Module(body=keep, type_ignores=[])
    ast.fix_missing_locations(mod)
    exec(compile(mod, path, "exec"), ns)


def curve_length_cv(points):
    """cv2.arcLength(np.asarray(points, np.single), False), restated"""
    p = np.asarray(points, np.float32).reshape(-1, 2)
    d = p[1:] - p[:-1]
    seg = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    return float(np.cumsum(seg.astype(np.float64))[-1]) if len(seg) else 0.0


def load_reference(root):
    import itertools
    import math
    import types

    from scipy import spatial
    np_shim = types.ModuleType("np_shim")
    np_shim.__dict__.update(np.__dict__)
    np_shim.int = np.int64
    it_shim = types.ModuleType("itertools_shim")
    it_shim.__dict__.update(itertools.__dict__)
    it_shim.izip = zip
    cv2_shim = types.ModuleType("cv2_shim")

    def arc_length(pts, closed):
        assert not closed, "only open curves are measured here"
        return curve_length_cv(pts)
    cv2_shim.arcLength = arc_length
    a = os.path.join(root, "video", "analysis")
    curves_ns = {"np": np_shim, "itertools": it_shim, "math": math, "cv2": cv2_shim, "__name__": "ref_curves"}
    _lift(os.path.join(a, "curves.py"), ("point_distance", "translate_points", "curve_length",
                                         "curve_segment_lengths", "make_curve_equidistant"), curves_ns)
    image_ns = {"np": np_shim, "__name__": "ref_image"}
    _lift(os.path.join(a, "image.py"), ("subpixel", "subpixels"), image_ns)
    curves_mod, image_mod = types.ModuleType("curves"), types.ModuleType("image")
    curves_mod.__dict__.update(curves_ns)
    image_mod.__dict__.update(image_ns)
    ac_ns = {"np": np_shim, "spatial": spatial, "curves": curves_mod, "image": image_mod, "xrange": range,
             "DictFiniteCapacity": lambda capacity: dict(), "__name__": "ref_active_contour"}
    _lift(os.path.join(a, "active_contour.py"), ("ActiveContour",), ac_ns)
    return ac_ns["ActiveContour"], curves_mod, image_mod


# ------------------------------------------------------------------------------------------ cases
HELPER_CURVES = {
    "wiggle": np.array([[0.0, 0.0], [3.0, 4.0], [3.5, 4.25], [10.0, -1.0], [10.0, -1.0], [12.75, 7.125],
                        [40.2, 7.1]]),
    "ellipse": ellipse_curve(37, True),
    "int": np.array([[0, 0], [5, 0], [5, 7], [1, 9]], np.int64),
}


def helper_cases(C, I, data):
    for name, c in HELPER_CURVES.items():
        data["curves/%s/in" % name] = c
        data["curves/%s/length" % name] = np.float64(C.curve_length(c))
        data["curves/%s/segments" % name] = C.curve_segment_lengths(c)
        data["curves/%s/equidistant" % name] = np.asarray(C.make_curve_equidistant(c))
        data["curves/%s/equidistant_count" % name] = np.asarray(C.make_curve_equidistant(c, count=11))
        data["curves/%s/equidistant_spacing" % name] = np.asarray(C.make_curve_equidistant(c, spacing=2.5))
        data["curves/%s/translated" % name] = np.asarray(C.translate_points(c, 1.5, -2.0))
        data["curves/%s/distance01" % name] = np.float64(C.point_distance(c[0], c[1]))
    img = sobel_input(9, 11, np.float32).astype(np.float64)
    pts = np.array([[0.0, 0.0], [0.5, 0.25], [3.7, 6.2], [9.0, 7.999], [8.99, 0.0], [4.0, 4.0]])
    data["image/img"] = img
    data["image/pts"] = pts
    data["image/subpixels"] = I.subpixels(img, pts)
    data["image/subpixel"] = np.array([I.subpixel(img, p) for p in pts])


MATRIX_CASES = [(N, ds, params, closed) for N in (3, 4, 5, 64) for ds in (0.75, 2.5)
                for params in ("ref", "centre") for closed in (False, True)]


def matrix_cases(AC, data):
    for N, ds, params, closed in MATRIX_CASES:
        pr = dict(PARAMS[params])
        pr.pop("blur_radius")
        P = AC(blur_radius=0, closed_loop=closed, **pr).get_evolution_matrix(N, ds)
        data["matrix/%d_%g_%s_%d" % (N, ds, params, closed)] = P


def sobel_cases(data):
    for dt, tag in ((np.uint8, "u8"), (np.float32, "f32")):
        for h, w in SOBEL_SIZES:
            x = sobel_input(h, w, dt, salt=h * 31 + w)
            fx, fy = sobel5(x)
            key = "sobel/%s_%dx%d" % (tag, h, w)
            data[key + "/fx"], data[key + "/fy"] = fx, fy
        p = sobel_input(48, 64, dt, salt=5)
        for s in BLUR_SIGMAS:
            fx, fy = gradients(p, s)
            key = "grad/%s_48x64_s%g" % (tag, s)
            for k, v in (("fx", fx), ("fy", fy)):
                data[key + "/" + k + "_sha"] = sha(v)
                data[key + "/" + k + "_sample"] = v.reshape(-1)[::7].copy()
    h, w, s = BIG
    fx, fy = gradients(big_input(), s)
    for k, v in (("fx", fx), ("fy", fy)):
        data["grad/big/" + k + "_sha"] = sha(v)
        data["grad/big/" + k + "_sample"] = v.reshape(-1)[::SAMPLE_STRIDE].copy()


def big_input():
    h, w, _ = BIG
    return (ramp((h, w), 77).astype(np.float32) * np.float32(0.5) + np.float32(3.25)).astype(np.float32)


def snake_cases(AC, C, data):
    grads = {}
    kept, dropped = [], []
    for name, pot, params, closed, N, max_it, ax, ay, kind in SNAKE_CASES:
        pr = PARAMS[params]
        gkey = (pot, pr["blur_radius"])
        if gkey not in grads:
            grads[gkey] = gradients(potential(pot), pr["blur_radius"])
        fx, fy = grads[gkey]
        curve = case_curve(N, closed, kind)
        anchor_x, anchor_y = case_anchor(ax, N), case_anchor(ay, N)
        ac = AC(closed_loop=closed, **pr)
        ac.max_iterations = max_it
        ac.residual_tolerance = TOLERANCE.get(name, 1)
        ac.fx, ac.fy = fx, fy
        sentinel = {"iteration_count": -7, "total_variation": -7.0}
        ac.info = dict(sentinel)
        out = np.asarray(ac.find_contour(curve, anchor_x=anchor_x, anchor_y=anchor_y))
        key = "snake/" + name
        if N > 2:
            # the restatement on the reference's own preparation, for the margin
            pts = np.asarray(C.make_curve_equidistant(curve))
            ds = C.curve_length(pts) / (len(pts) - 1)
            Pinv = ac.get_evolution_matrix(len(pts), ds)
            flags, vals = restated_anchors(curve, pts, anchor_x, anchor_y)
            _, _, _, margin = snake(fx, fy, pts, Pinv, ac.gamma, ac.residual_tolerance * ac.gamma, max_it,
                                    flags, vals)
            if margin < MIN_MARGIN:
                dropped.append((name, margin))
                continue
            data[key + "/margin"] = np.float64(margin)
            data[key + "/iterations"] = np.int64(ac.info["iteration_count"])
            data[key + "/total_variation"] = np.float64(ac.info["total_variation"])
        else:
            assert ac.info == sentinel
        data[key + "/curve"] = curve
        data[key + "/points"] = out
        kept.append(name)
    return kept, dropped


def restated_anchors(curve, points, anchor_x, anchor_y):
    """the anchors as ActiveContour._anchors arranges them for the kernel (cdist argmin, last wins)"""
    if anchor_x is None and anchor_y is None:
        return None, None
    flags = np.zeros(len(points), np.uint8)
    vals = np.zeros((len(points), 2))
    for coord, indices in ((0, anchor_x), (1, anchor_y)):
        if indices is None or len(indices) == 0:
            continue
        ps = np.asarray(curve)[indices, :]
        d = points[:, None, :] - np.asarray(ps, np.float64)[None, :, :]
        idx = np.argmin(np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]), axis=0)
        vals[idx, coord] = ps[:, coord]
        flags[idx] |= np.uint8(1 << coord)
    return flags, vals


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("VA_REFERENCE")
    if not root or not os.path.isdir(os.path.join(root, "video", "analysis")):
        sys.stderr.write("usage: make_golden_active_contour.py <reference checkout> (or $VA_REFERENCE); "
                         "nothing written\n")
        raise SystemExit(2)
    AC, C, I = load_reference(root)
    data = {"shims": np.array(SHIMS)}
    helper_cases(C, I, data)
    matrix_cases(AC, data)
    sobel_cases(data)
    kept, dropped = snake_cases(AC, C, data)
    if dropped:
        sys.stderr.write("dropped (margin < %g): %s\n" % (MIN_MARGIN, dropped))
    data["snake_kept"] = np.array(kept)
    np.savez_compressed(OUT, **data)
    print("wrote %s (%d arrays, %d snake cases kept, %d dropped, %d bytes)"
          % (OUT, len(data), len(kept), len(dropped), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
