"""The scalar restatement of curves.make_curve_equidistant ("Equidistant curves") and the curves
the curve tests share.  The restatement is written with Python floats (IEEE double, one rounding an operation),
np.float32 scalars and exact rationals: it uses none of np.linalg.norm, math.hypot, np.interp and np.linspace,
which are what it is compared with."""
import ctypes as C
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ----------------------------------------------------------------------------------------- the restatement
def fma(a, b, c):
    """a * b + c with one rounding (the exact rational, rounded once by float())"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def norm2(dx, dy):
    """np.linalg.norm of a 2-vector on a BLAS with FMA: the x product rounded, the y product fused into the sum"""
    return math.sqrt(fma(dy, dy, dx * dx))


def sqrt_exact(q):
    """the correctly rounded double root of a non-negative rational: an integer root with 130 bits or more and a
    sticky bit, rounded once"""
    if q == 0:
        return 0.0
    num, den = q.numerator, q.denominator
    shift = max(0, 260 - (num.bit_length() - den.bit_length()))
    shift += shift & 1
    scaled = (num << shift) // den
    exact = (scaled * den == num << shift)
    r = math.isqrt(scaled)
    exact = exact and r * r == scaled
    return float(Fraction(2 * r + (0 if exact else 1), 1 << (shift // 2 + 1)))


def hypot(a, b):
    """the correctly rounded sqrt(a*a + b*b)"""
    return sqrt_exact(Fraction(a) ** 2 + Fraction(b) ** 2)


def length_f32(points):
    """curves.curve_length: float32 casts, float32 dx*dx + dy*dy and root, the roots added in double in order"""
    p = [(np.float32(x), np.float32(y)) for x, y in points]
    total = 0.0
    for (x1, y1), (x2, y2) in zip(p, p[1:]):
        dx, dy = np.float32(x2 - x1), np.float32(y2 - y1)
        s = np.float32(np.float32(dx * dx) + np.float32(dy * dy))
        total += float(np.float32(math.sqrt(float(s))))       # (the double root of a float rounds to the float root)
    return total


def rint(v):
    """round half to even"""
    f = math.floor(v)
    d = v - f
    if d > 0.5 or (d == 0.5 and f % 2 == 1):
        return f + 1.0
    return float(f)


def equidistant(points, spacing=None, count=None, offset=None):
    """the pinned definition, scalar by scalar; returns a (K, 2) float64 array"""
    P = [(float(x), float(y)) for x, y in np.asarray(points, np.double).reshape(-1, 2)]
    n = len(P)
    if spacing is not None:
        spacing = float(spacing)
        L = length_f32(P)
        if L < spacing:
            out = list(P)
        else:
            dx = L / rint(L / spacing)
            out = [P[0]]
            dist = 0.0
            for (p1x, p1y), (p2x, p2y) in zip(P, P[1:]):
                dp = norm2(p2x - p1x, p2y - p1y)
                while dist + dp > dx:
                    f = (dx - dist) / dp
                    p1x, p1y = p1x + f * (p2x - p1x), p1y + f * (p2y - p1y)
                    out.append((p1x, p1y))
                    dp = norm2(p2x - p1x, p2y - p1y)
                    dist = 0.0
                dist += dp
            if dist > 1e-8:
                out.append(P[-1])
    else:
        count = n if count is None else int(count)
        s = [0.0]
        for (x1, y1), (x2, y2) in zip(P, P[1:]):
            s.append(s[-1] + hypot(x1 - x2, y1 - y2))
        step = s[-1] / (count - 1) if count > 1 else 0.0
        out = []
        j = 0
        for k in range(count):
            x = s[-1] if (count > 1 and k == count - 1) else k * step + 0.0
            if x >= s[-1]:
                out.append(P[-1])
                continue
            while s[j + 1] <= x:                 # j: the last index with s[j] <= x (x < s[-1] ends the search)
                j += 1
            if x == s[j]:
                out.append(P[j])
                continue
            pt = []
            for c in (0, 1):
                slope = (P[j + 1][c] - P[j][c]) / (s[j + 1] - s[j])
                pt.append(slope * (x - s[j]) + P[j][c])
            out.append(tuple(pt))
    res = np.array(out, np.float64).reshape(-1, 2)
    if offset is not None:
        res = np.array([(x + float(offset[0]), y + float(offset[1])) for x, y in res], np.float64).reshape(-1, 2)
    return res


# ----------------------------------------------------------------------------------------- shared curves
def pixel_path(rng, n):
    """an 8-connected integer path of n points that mostly keeps its heading, as a skeleton's branch does"""
    steps = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]
    h = int(rng.integers(8))
    pts = [(int(rng.integers(5, 60)), int(rng.integers(5, 60)))]
    for _ in range(n - 1):
        h = (h + int(rng.choice((-1, 0, 0, 0, 1)))) % 8
        pts.append((pts[-1][0] + steps[h][0], pts[-1][1] + steps[h][1]))
    return np.array(pts, np.int64)


def float_curve(rng, n, scale=10.0, offset=0.0):
    """a random walk of n float points with steps of about `scale`, around `offset`"""
    return np.cumsum(rng.normal(0, scale, (n, 2)), axis=0) + offset


def mixed_curves(seed, m, lo=2, hi=300):
    """m curves of lo..hi points: pixel paths, float walks and float walks near 1000"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(m):
        n = int(rng.integers(lo, hi + 1))
        kind = k % 3
        out.append(pixel_path(rng, n) if kind == 0 else float_curve(rng, n, 3.0) if kind == 1
                   else float_curve(rng, n, 1.5, 1000.0))
    return out


def fixture_curves():
    """the three curves of tests/golden/active_contour_v1.npz"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "active_contour_v1.npz"))
    names = sorted(set(k.split("/")[1] for k in z.files if k.startswith("curves/")))
    return {name: z["curves/%s/in" % name] for name in names}, z


# ----------------------------------------------------------------------------------------- the compiled header
def compile_shim(tmpdir):
    """tests/curves_shim.cpp + va_curves_math.h as a shared object under tmpdir, bound with ctypes; None without
    a host C++ compiler"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        return None
    so = os.path.join(str(tmpdir), "libcurves_shim.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "video-analysis_amd", "csrc"),
                           os.path.join(ROOT, "tests", "curves_shim.cpp"), "-o", so, "-lm"])
    lib = C.CDLL(so)
    vp, i64, d, i = C.c_void_p, C.c_int64, C.c_double, C.c_int
    lib.cs_hypot.argtypes = lib.cs_norm2.argtypes = [vp, vp, vp, i64]
    lib.cs_hypot.restype = lib.cs_norm2.restype = None
    lib.cs_length_f32.argtypes, lib.cs_length_f32.restype = [vp, i64], d
    lib.cs_spacing_count.argtypes, lib.cs_spacing_count.restype = [vp, i64, d, i64], i64
    lib.cs_spacing_store.argtypes, lib.cs_spacing_store.restype = [vp, i64, d, i, d, d, vp, i64, vp], i64
    lib.cs_arc_total.argtypes, lib.cs_arc_total.restype = [vp, i64], d
    lib.cs_count_store.argtypes, lib.cs_count_store.restype = [vp, i64, i64, i, d, d, vp, vp], None
    return lib


def shim_equidistant(lib, points, spacing=None, count=None, offset=None):
    """the header's result for one curve: ((K, 2) points, float32-rule length of the output)"""
    P = np.ascontiguousarray(points, np.float64).reshape(-1, 2)
    n = len(P)
    shift, (tx, ty) = int(offset is not None), (offset if offset is not None else (0.0, 0.0))
    length = C.c_double()
    if spacing is not None:
        k = lib.cs_spacing_count(P.ctypes.data, n, float(spacing), 1 << 30)
        out = np.empty((k, 2), np.float64)
        got = lib.cs_spacing_store(P.ctypes.data, n, float(spacing), shift, float(tx), float(ty), out.ctypes.data, k,
                                   C.byref(length))
        assert got == k
    else:
        k = n if count is None else int(count)
        out = np.empty((k, 2), np.float64)
        lib.cs_count_store(P.ctypes.data, n, k, shift, float(tx), float(ty), out.ctypes.data, C.byref(length))
    return out, length.value
