"""The scalar restatements of the two pinned simplifiers ("Simplification") and the curves the
simplification tests share.  The restatements are written with Python floats (IEEE double, one rounding an
operation) and plain lists: Ramer-Douglas-Peucker with the pinned distance, and the Visvalingam procedure of the
reference's external/simplify_polygon_visvalingam.py restated by index -- a heap array of point indices, prev / next
arrays and CPython heapq's two sift procedures, the areas measured afresh at every comparison."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESHOLDS = (0, 0.5, 2, 10, 200, 1e9)


def _points(curve):
    return [(float(x), float(y)) for x, y in np.asarray(curve, np.float64).reshape(-1, 2)]


# ------------------------------------------------------------------------------------- Ramer-Douglas-Peucker
def chord_distance(x0, x1, x2):
    """the pinned distance of x0 from the chord x1 -> x2"""
    if x1[0] == x2[0]:
        return abs(x0[0] - x1[0])
    ax, ay = x2[0] - x1[0], x2[1] - x1[1]
    bx, by = x1[0] - x0[0], x1[1] - x0[1]
    p, q = ax * by, ay * bx
    u, v = ax * ax, ay * ay
    return abs(p - q) / math.sqrt(u + v)


def span_farthest(P, i0, i1):
    """(largest distance above 0, the first index that has it or None) of the points strictly inside (i0, i1)"""
    best, index = 0.0, None
    for i in range(i0 + 1, i1):
        d = chord_distance(P[i], P[i0], P[i1])
        if d > best:
            best, index = d, i
    return best, index


def rdp_keep(curve, eps):
    """the kept flags (uint8, one per point) of the pinned Ramer-Douglas-Peucker; the spans are taken first in,
    first out, another order than the kernel's and the header's"""
    P = _points(curve)
    n = len(P)
    keep = np.zeros(n, np.uint8)
    if n < 3:
        keep[:] = 1
        return keep
    keep[0] = keep[n - 1] = 1
    tol = eps if eps > 0 else 0.0
    todo = [(0, n - 1)]
    while todo:
        i0, i1 = todo.pop(0)
        if i1 - i0 < 2:
            continue
        d, k = span_farthest(P, i0, i1)
        if d > tol:
            keep[k] = 1
            todo += [(i0, k), (k, i1)]
    return keep


# ------------------------------------------------------------------------------------- Visvalingam
def triangle_area(p1, p2, p3):
    return abs(p1[0] * (p2[1] - p3[1]) + p2[0] * (p3[1] - p1[1]) + p3[0] * (p1[1] - p2[1])) / 2.0


class _Heap(object):
    """the heap of point indices with its links; less(a, b) measures both areas now"""

    def __init__(self, P, closed):
        n = len(P)
        self.P = P
        self.prev = [i - 1 if i > 0 else (n - 1 if closed else 0) for i in range(n)]
        self.next = [i + 1 if i + 1 < n else (0 if closed else n - 1) for i in range(n)]
        self.heap = list(range(n)) if closed else list(range(1, n - 1))

    def area(self, i):
        return triangle_area(self.P[i], self.P[self.prev[i]], self.P[self.next[i]])

    def less(self, a, b):
        return self.area(a) < self.area(b)

    def siftdown(self, startpos, pos):                       # heapq._siftdown
        heap = self.heap
        newitem = heap[pos]
        while pos > startpos:
            parentpos = (pos - 1) >> 1
            parent = heap[parentpos]
            if self.less(newitem, parent):
                heap[pos] = parent
                pos = parentpos
                continue
            break
        heap[pos] = newitem

    def siftup(self, pos):                                   # heapq._siftup
        heap = self.heap
        endpos = len(heap)
        startpos = pos
        newitem = heap[pos]
        childpos = 2 * pos + 1
        while childpos < endpos:
            rightpos = childpos + 1
            if rightpos < endpos and not self.less(heap[childpos], heap[rightpos]):
                childpos = rightpos
            heap[pos] = heap[childpos]
            pos = childpos
            childpos = 2 * pos + 1
        heap[pos] = newitem
        self.siftdown(startpos, pos)

    def run(self, thr, floor):
        heap = self.heap
        for i in reversed(range(len(heap) // 2)):            # heapq.heapify
            self.siftup(i)
        while len(heap) > floor:
            top = heap[0]
            if self.area(top) >= thr:
                break
            b, a = self.prev[top], self.next[top]
            self.next[b] = a
            self.prev[a] = b
            last = heap.pop()                                # heapq.heappop
            if heap:
                heap[0] = last
                self.siftup(0)
        return heap


def visvalingam(curve, thr, closed):
    """(kept flags uint8, the heap as it is left) of one ring (no closing duplicate) or one open line.  A ring of
    fewer than 3 points, or left with fewer than 3, keeps none: the reference's None"""
    P = _points(curve)
    n = len(P)
    keep = np.zeros(n, np.uint8)
    if n < 3:
        keep[:] = 0 if closed else 1
        return keep, []
    heap = _Heap(P, closed).run(float(thr), 2 if closed else 0)
    if closed and len(heap) < 3:
        return keep, heap
    keep[heap] = 1
    if not closed:
        keep[0] = keep[n - 1] = 1
    return keep, heap


def visvalingam_keep(curve, thr, closed):
    return visvalingam(curve, thr, closed)[0]


def simplified(curve, tolerance, method="rdp", closed=False):
    """the restatement's result in the form ops.simplify_curves returns: the kept rows of the curve as it was given,
    None for a ring that vanishes"""
    a = np.asarray(curve)
    keep = rdp_keep(a, tolerance) if method == "rdp" else visvalingam_keep(a, tolerance, closed)
    if method != "rdp" and closed and not keep.any():
        return None
    return a.reshape(-1, 2)[keep.astype(bool)]


def same_result(got, want):
    """both None, or arrays of one dtype and shape with equal bytes"""
    if got is None or want is None:
        return got is None and want is None
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------- shared curves
def integer_contour(rng, n):
    """a closed integer outline of n points: a circle of random radius with integer noise, as find_contours gives"""
    t = np.linspace(0, 2 * np.pi, n, endpoint=False)
    r = rng.uniform(4, 40) + rng.integers(-2, 3, n)
    return np.stack([np.rint(60 + r * np.cos(t)), np.rint(60 + r * np.sin(t))], 1).astype(np.int64)


def staircase(rng, n):
    """unit steps, right or up or down: one point per step"""
    steps = np.array([(1, 0), (0, 1), (1, 0), (0, -1)])[rng.integers(0, 4, n - 1)] if n > 1 else np.zeros((0, 2), int)
    return np.concatenate([[(3, 7)], (3, 7) + np.cumsum(steps, 0)]).astype(np.int64)[:n]


def noisy_circle(rng, n):
    t = np.linspace(0, 2 * np.pi, n, endpoint=False)
    r = 25 + rng.normal(0, 1.5, n)
    return np.stack([100.5 + r * np.cos(t), 80.25 + r * np.sin(t)], 1)


def float_walk(rng, n, scale=3.0):
    return np.cumsum(rng.normal(0, scale, (n, 2)), axis=0)


def random_curve(rng, n):
    """one of the four kinds above, by turns of the generator"""
    kind = int(rng.integers(4))
    return (integer_contour, staircase, noisy_circle, float_walk)[kind](rng, n)


def random_curves(seed, m, lo=3, hi=120):
    rng = np.random.default_rng(seed)
    return [random_curve(rng, int(rng.integers(lo, hi + 1))) for _ in range(m)]


_FIXTURE = []


def fixture():
    """tests/golden/simplify_v1.npz, what the reference's simplify_ring and simplify_line returned: a list of
    (name, input curve, closed, threshold, kept points or None), read once"""
    if not _FIXTURE:
        z = np.load(os.path.join(ROOT, "tests", "golden", "simplify_v1.npz"))
        for name in (str(s) for s in z["names"]):
            for mode in ("ring", "line"):
                if "%s/%s/counts" % (mode, name) not in z.files:
                    continue
                points, at = z["%s/%s/points" % (mode, name)], 0
                for thr, count in zip(z["thresholds"].tolist(), z["%s/%s/counts" % (mode, name)].tolist()):
                    want = None if count < 0 else points[at:at + count]
                    at += max(count, 0)
                    _FIXTURE.append((name, z["in/" + name], mode == "ring", thr, want))
    return _FIXTURE


def rdp_fixture():
    """the 27 rdp/<name>/<eps> entries of tests/golden/skeleton_graph_v1.npz, written by the reference's own rdp:
    a list of (name, input curve, eps, result)"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "skeleton_graph_v1.npz"))
    out = []
    for key in z.files:
        if key.startswith("rdp/"):
            _, name, eps = key.split("/")
            out.append((name, z["rdp_in/" + name], float(eps), z[key]))
    return out


# ------------------------------------------------------------------------------------- the compiled header
def compile_shim(tmpdir):
    """tests/simplify_shim.cpp + va_simplify_math.h as a shared object under tmpdir, bound with ctypes; None without
    a host C++ compiler"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        return None
    so = os.path.join(str(tmpdir), "libsimplify_shim.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "video-analysis_amd", "csrc"),
                           os.path.join(ROOT, "tests", "simplify_shim.cpp"), "-o", so, "-lm"])
    lib = C.CDLL(so)
    vp, i64, d, i = C.c_void_p, C.c_int64, C.c_double, C.c_int
    lib.ss_chord_distance.argtypes = lib.ss_triangle_area.argtypes = [vp, vp, i64]
    lib.ss_chord_distance.restype = lib.ss_triangle_area.restype = None
    lib.ss_span_farthest.argtypes, lib.ss_span_farthest.restype = [vp, i, i, i, vp], i
    lib.ss_rdp_keep.argtypes, lib.ss_rdp_keep.restype = [vp, i, d, vp], i
    lib.ss_visvalingam_heap.argtypes, lib.ss_visvalingam_heap.restype = [vp, i, d, i, vp, vp, vp], i
    lib.ss_visvalingam_keep.argtypes, lib.ss_visvalingam_keep.restype = [vp, i, d, i, vp, vp, vp, vp], i
    return lib


def shim_rdp(lib, curve, eps):
    """(kept flags, count) of the header's serial Ramer-Douglas-Peucker"""
    P = np.ascontiguousarray(curve, np.float64).reshape(-1, 2)
    keep = np.full(len(P), 0xA5, np.uint8)
    return keep, lib.ss_rdp_keep(P.ctypes.data, len(P), float(eps), keep.ctypes.data)


def shim_visvalingam(lib, curve, thr, closed):
    """(kept flags, count, heap as it is left) of the header's Visvalingam, its tables dirty beforehand"""
    P = np.ascontiguousarray(curve, np.float64).reshape(-1, 2)
    n = len(P)
    keep = np.full(n, 0xA5, np.uint8)
    tables = [np.full(max(n, 1), -1515870811, np.int32) for _ in range(3)]
    count = lib.ss_visvalingam_keep(P.ctypes.data, n, float(thr), int(closed), tables[0].ctypes.data,
                                    tables[1].ctypes.data, tables[2].ctypes.data, keep.ctypes.data)
    heap = []
    if n >= 3:
        left = lib.ss_visvalingam_heap(P.ctypes.data, n, float(thr), int(closed), tables[0].ctypes.data,
                                       tables[1].ctypes.data, tables[2].ctypes.data)
        heap = tables[0][:left].tolist()
    return keep, count, heap
