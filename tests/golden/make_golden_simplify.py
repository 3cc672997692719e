#!/usr/bin/env python3
"""Generates tests/golden/simplify_v1.npz -- simplify_ring and simplify_line of the reference's
external/simplify_polygon_visvalingam.py (behind regions.simplify_contour, video/analysis/regions.py:307-325) as the
reference's own code computes them, on rings and open lines at the thresholds 0, 0.5, 2, 10, 200 and 1e9.

    python tests/golden/make_golden_simplify.py <reference checkout>      (or set $VA_REFERENCE)

Importing this module needs no checkout: it holds the case table (`cases`) alone.  The restatement the results
are compared with lives in tests/simplify_checks.py.  Writing the fixture lifts the reference's module at run time
and runs it in a namespace of shims; none of its source is stored, only the curves and what it returned.

Shims, and why none of them can change a result:
  the shapely imports          stripped: shapely is not installed, and the two functions use it only to build the
                               object they return
  print "ERROR:"               the Python 2 statement is rewritten as a call before parsing; it never runs
  TriangleCalculator.__lt__    area(a) < area(b): what Python 2's heapq makes of the class's __cmp__
  LinearRing, LineString       classes with `.coords`, a list of float tuples; the ring appends its first point
                               when the last differs, as shapely's does, and remembers the list it was given
The recorded result of a ring is the list simplify_ring hands to LinearRing -- the kept points in order, before the
ring is closed again -- or None; of a line, the coordinates of the LineString.  Every case is compared exactly with
the restatement while the fixture is written; none is dropped.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "simplify_v1.npz")


def _checks():
    spec = importlib.util.spec_from_file_location("simplify_checks", os.path.join(os.path.dirname(HERE),
                                                                                   "simplify_checks.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cases():
    """[(name, (n, 2) curve, modes)]: modes names what the curve is run as, 'ring', 'line' or both"""
    K = _checks()
    rng = np.random.default_rng(20240611)
    out = []
    for n in (5, 12, 30, 64, 65, 100, 200):
        out.append(("contour%d" % n, K.integer_contour(rng, n), ("ring", "line") if n in (12, 65) else ("ring",)))
    for n in (3, 10, 33, 64, 129, 200):
        out.append(("stairs%d" % n, K.staircase(rng, n), ("ring", "line") if n in (10, 129) else ("line",)))
    for n in (8, 40, 63, 128, 199):
        out.append(("circle%d" % n, K.noisy_circle(rng, n), ("ring", "line") if n == 40 else ("ring",)))
    for n in (3, 4, 20, 77):
        out.append(("walk%d" % n, K.float_walk(rng, n), ("line", "ring") if n == 20 else ("line",)))
    for n in (16, 50, 90, 150):
        out.append(("stairs_ring%d" % n, K.staircase(rng, n), ("ring",)))
    for n in (6, 25, 70, 180):
        out.append(("contour_line%d" % n, K.integer_contour(rng, n), ("line",)))
    for n in (7, 31, 110):
        out.append(("circle_line%d" % n, K.noisy_circle(rng, n), ("line",)))
    ring = K.integer_contour(rng, 24)
    out.append(("repeated", np.repeat(ring, [1, 2, 1, 3] * 6, axis=0), ("ring", "line")))
    out.append(("collinear", np.stack([np.arange(9), 2 * np.arange(9) + 1], 1).astype(np.int64), ("ring", "line")))
    out.append(("tri", np.array([[0, 0], [7, 1], [3, 9]], np.int64), ("ring", "line")))
    out.append(("quad", np.array([[0.5, 0.25], [6.0, 1.0], [7.5, 8.0], [1.0, 5.5]]), ("ring", "line")))
    out.append(("square_in_steps", np.array([[0, 0], [1, 0], [2, 0], [2, 1], [2, 2], [1, 2], [0, 2], [0, 1]],
                                            np.int64), ("ring", "line")))
    return out


# ------------------------------------------------------------------------------------- the lifted module
class LinearRing(object):
    def __init__(self, coords):
        self.given = [tuple(float(v) for v in p) for p in coords]
        self.coords = list(self.given)
        if self.coords and self.coords[-1] != self.coords[0]:
            self.coords.append(self.coords[0])


class LineString(object):
    def __init__(self, coords):
        self.coords = [tuple(float(v) for v in p) for p in coords]


def lift(root):
    """the reference's module, executed in a namespace of the shims above: (simplify_ring, simplify_line)"""
    path = os.path.join(root, "external", "simplify_polygon_visvalingam.py")
    text = open(path).read()
    lines = [ln for ln in text.split("\n") if not ln.startswith("from shapely")]
    text = "\n".join(lines).replace('print "ERROR:"', 'print("ERROR:")')
    space = {"LinearRing": LinearRing, "LineString": LineString, "__name__": "lifted_visvalingam"}
    exec(compile(text, path, "exec"), space)
    space["TriangleCalculator"].__lt__ = lambda a, b: a.calcArea() < b.calcArea()
    return space["simplify_ring"], space["simplify_line"]


def generate(root):
    K = _checks()
    simplify_ring, simplify_line = lift(root)
    data = {"thresholds": np.array(K.THRESHOLDS, np.float64)}
    names, vanished, nothing_removed = [], 0, 0
    for name, curve, modes in cases():
        assert tuple(curve[0]) != tuple(curve[-1]), name          # (no closing duplicate: the ring shim appends one)
        names.append(name)
        data["in/" + name] = curve
        for mode in modes:
            # per curve and mode: the results at the six thresholds one after the other, and their point counts
            # (-1: None)
            rows, counts = [], []
            for thr in K.THRESHOLDS:
                key = "%s/%s/%g" % (mode, name, thr)
                if mode == "ring":
                    res = simplify_ring(LinearRing(curve), thr)
                    pts = None if res is None else res.given
                else:
                    pts = simplify_line(LineString(curve), thr).coords
                want = K.simplified(np.asarray(curve, np.float64), thr, "visvalingam", closed=(mode == "ring"))
                if pts is None:
                    assert want is None, key
                    vanished += 1
                    counts.append(-1)
                    continue
                assert want is not None and [tuple(p) for p in want.tolist()] == list(pts), key
                nothing_removed += len(pts) == len(curve)
                rows += list(pts)
                counts.append(len(pts))
            data["%s/%s/points" % (mode, name)] = np.array(rows, np.float64).reshape(-1, 2).astype(curve.dtype)
            data["%s/%s/counts" % (mode, name)] = np.array(counts, np.int32)
    data["names"] = np.array(names)
    assert vanished and nothing_removed
    return data


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("VA_REFERENCE")
    if not root or not os.path.isfile(os.path.join(root, "external", "simplify_polygon_visvalingam.py")):
        sys.stderr.write("usage: make_golden_simplify.py <reference checkout> (or $VA_REFERENCE); nothing written\n")
        raise SystemExit(2)
    data = generate(root)
    np.savez_compressed(OUT, **data)
    print("wrote %s (%d arrays, %d bytes)" % (OUT, len(data), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
