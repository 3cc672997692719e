#!/usr/bin/env python3
"""Generates tests/golden/outline_v1.npz -- get_ray_hitpoint, get_ray_intersections and
get_farthest_ray_intersection (video/analysis/regions.py:353-426) as the reference's own code computes them over the
NumPy restatement of the pinned outline queries ("Outline queries"), and the restated containment of
Polygon.contains (video/analysis/shapes.py:552-554).

    python tests/golden/make_golden_outline.py <reference checkout>      (or set $VA_REFERENCE)

Importing this module needs no checkout: the tests take the restatement (`ray_edges`, `ray_hit`, `ray_hits`,
`contains`, `contains_points`, `point_distance` and, built on them, `get_ray_hitpoint` and
`get_farthest_ray_intersection`), the case tables and the seeded generators (`outlines`, `star_ring`) from it.  Writing the fixture lifts the reference's three
ray functions with make_golden_polygon._lift at run time and runs them in a namespace of shims; none of their
source is stored.

Shims, and why none of them can change a result:
  geometry.LineString, .intersection    the restatement: an outline's intersection with a ray is a `Point` at the
                                        hit of the smallest (t, i), or an empty geometry (shapely is not installed;
                                        agreement with GEOS is expected and unverified)
  geometry.Point, geos.TopologicalError the classes the reference tests its result against; nothing raises
  curves.point_distance                 the pinned distance sqrt(dx dx + dy dy); the reference's math.hypot differs
                                        from it by at most one unit in the last place (a listed deviation)
The reference's own control flow produces the recorded results: the angle loop, the far points, the strict maximum
and the None / nan returns.  Every case is compared exactly; none is dropped.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "outline_v1.npz")


def _sibling(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------- restatement
def _points(pts):
    p = np.asarray(pts, np.float64)
    return p.reshape(0, 2) if p.size == 0 else p


def edge_count(n, closed):
    return 0 if n == 0 else (n if closed else n - 1)


def ray_edges(anchor, far, pts, closed):
    """(t, hit) per edge of the outline: edge i runs from point i to point i + 1, the closing edge from the last
    point to the first.  Plain float64 NumPy operations, each rounded on its own."""
    P = _points(pts)
    n = len(P)
    i = np.arange(edge_count(n, closed))
    Pi, Qi = P[i], P[(i + 1) % max(n, 1)]
    a, f = np.asarray(anchor, np.float64), np.asarray(far, np.float64)
    with np.errstate(all="ignore"):
        dx, dy = f[0] - a[0], f[1] - a[1]
        ex, ey = Qi[:, 0] - Pi[:, 0], Qi[:, 1] - Pi[:, 1]
        wx, wy = Pi[:, 0] - a[0], Pi[:, 1] - a[1]
        den = dx * ey - dy * ex
        tn = wx * ey - wy * ex
        un = wx * dy - wy * dx
        t, u = tn / den, un / den
        hit = (den != 0) & (t >= 0) & (t <= 1) & (u >= 0) & (u <= 1)
    return t, hit


def ray_hit(anchor, far, pts, closed):
    """(t, (hx, hy), edge, count) of one ray: the hitting edge with the smallest (t, i); (nan, (nan, nan), -1, 0)
    without a hit"""
    t, hit = ray_edges(anchor, far, pts, closed)
    k = np.flatnonzero(hit)
    if not len(k):
        return np.float64(np.nan), (np.float64(np.nan), np.float64(np.nan)), -1, 0
    edge = int(k[np.flatnonzero(t[k] == t[k].min())[0]])
    a, f = np.asarray(anchor, np.float64), np.asarray(far, np.float64)
    with np.errstate(all="ignore"):
        dx, dy = f[0] - a[0], f[1] - a[1]
        h = (a[0] + t[edge] * dx, a[1] + t[edge] * dy)
    return t[edge], h, edge, len(k)


def ray_hits(outline_list, closed, anchors, fars, index):
    """the batch: (t (q,), hits (q, 2), edge int32 (q,), count int32 (q,))"""
    q = len(index)
    t, hits = np.full(q, np.nan), np.full((q, 2), np.nan)
    edge, count = np.full(q, -1, np.int32), np.zeros(q, np.int32)
    for k in range(q):
        o = int(index[k])
        t[k], hits[k], edge[k], count[k] = ray_hit(anchors[k], fars[k], outline_list[o], closed[o])
    return t, hits, edge, count


def point_distance(p1, p2):
    """the pinned distance: sqrt(dx dx + dy dy) in float64"""
    dx = np.float64(p1[0]) - np.float64(p2[0])
    dy = np.float64(p1[1]) - np.float64(p2[1])
    return np.sqrt(dx * dx + dy * dy)


def contains(pts, point):
    """the pinned containment of a point in the ring `pts`, closed with the edge from its last point to its first"""
    P = _points(pts)
    x, y = np.float64(point[0]), np.float64(point[1])
    if len(P) < 3 or not (np.isfinite(x) and np.isfinite(y)):
        return False
    Q = np.roll(P, -1, axis=0)
    px, py, qx, qy = P[:, 0], P[:, 1], Q[:, 0], Q[:, 1]
    with np.errstate(all="ignore"):
        c = (qx - px) * (y - py) - (qy - py) * (x - px)
    in_x = ((px <= x) & (x <= qx)) | ((qx <= x) & (x <= px))
    in_y = ((py <= y) & (y <= qy)) | ((qy <= y) & (y <= py))
    boundary = (c == 0) & in_x & in_y
    toggle = ~boundary & ((py > y) != (qy > y)) & np.where(qy > py, c > 0, c < 0)
    return bool(not boundary.any() and toggle.sum() % 2 == 1)


def contains_points(outline_list, points, index):
    return np.array([contains(outline_list[int(o)], p) for p, o in zip(points, index)], bool)


def get_ray_hitpoint(anchor, far, pts, closed, ret_dist=False):
    """the restated get_ray_hitpoint: a tuple of floats or None; with ret_dist (point, distance) or (None, nan)"""
    _, h, edge, _ = ray_hit(anchor, far, pts, closed)
    if edge < 0:
        return (None, np.nan) if ret_dist else None
    point = (float(h[0]), float(h[1]))
    return (point, float(point_distance(point, anchor))) if ret_dist else point


def get_farthest_ray_intersection(anchor, angles, pts, closed, ray_length=1000):
    """the restated get_farthest_ray_intersection: (hit points or None per angle, (point, distance, angle) of the
    farthest hit); starts from (None, 0, None) and replaces the best only on a strictly larger distance"""
    best, points = (None, 0, None), []
    for angle in angles:
        far = (anchor[0] + ray_length * np.cos(angle), anchor[1] + ray_length * np.sin(angle))
        point, dist = get_ray_hitpoint(anchor, far, pts, closed, ret_dist=True)
        points.append(point)
        if dist > best[1]:
            best = (point, dist, angle)
    return points, best


# --------------------------------------------------------------------------------------- generators
def star_ring(rng, n, centre=(50.0, 50.0), radii=(12.0, 40.0), step=None):
    """n points of a star-shaped ring about `centre` (sorted random directions, random radii); step: the grid the
    coordinates are rounded to (0.5: half-integers), None: as computed"""
    ang = np.sort(rng.uniform(0, 2 * np.pi, n))
    rad = rng.uniform(radii[0], radii[1], n)
    p = np.stack([centre[0] + rad * np.cos(ang), centre[1] + rad * np.sin(ang)], 1)
    return p if step is None else np.round(p / step) * step


SQUARE = [(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)]


def outlines():
    """name -> (points (n, 2) float64, closed) of the fixture: 28 outlines of up to 300 points"""
    rng = np.random.default_rng(21)
    out = {"unit_square": (np.array(SQUARE), True),
           "unit_square_open": (np.array(SQUARE), False),
           "unit_square_ring": (np.array(SQUARE + SQUARE[:1]), False),
           "box": (np.array([(10.0, 10.0), (90.0, 10.0), (90.0, 70.0), (10.0, 70.0)]), True),
           "notch": (np.array([(10.0, 10.0), (90.0, 10.0), (90.0, 70.0), (50.0, 30.0), (10.0, 70.0)]), True),
           "doubled": (np.array([(10.0, 10.0), (10.0, 10.0), (90.0, 10.0), (90.0, 70.0), (90.0, 70.0), (10.0, 70.0),
                                 (10.0, 10.0)]), False),
           "zigzag": (np.array([(float(5 * k), 20.0 + 30.0 * (k % 2)) for k in range(20)]), False),
           "segment": (np.array([(20.0, 80.0), (80.0, 20.0)]), False)}
    for k, n in enumerate((3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 300)):
        out["star_%d" % n] = (star_ring(rng, n, step=0.5 if k % 2 == 0 else None), True)
    for k, n in enumerate((4, 9, 17, 40, 77, 150)):
        p = star_ring(rng, n, step=None if k % 2 == 0 else 0.5)
        out["ring_%d" % n] = (np.concatenate([p, p[:1]]), False)
    for n in (6, 30, 120):
        out["arc_%d" % n] = (star_ring(rng, n)[: max(2, 2 * n // 3)], False)
    return out


# (outline, anchor, far) of the fixture's single rays, the known answers of the unit square among them
RAY_CASES = [
    ("unit_square", (0.5, 0.5), (2.0, 0.5)), ("unit_square_open", (0.5, 0.5), (-1.0, 0.5)),
    ("unit_square", (0.5, 0.5), (-1.0, 0.5)), ("unit_square", (0.0, 0.0), (2.0, 2.0)),
    ("unit_square", (0.5, 0.5), (1.5, 1.5)), ("unit_square", (-1.0, 0.0), (2.0, 0.0)),
    ("unit_square", (0.5, 0.5), (0.5, 0.5)), ("unit_square", (0.5, 0.5), (1.0, 0.5)),
    ("unit_square", (1.0, 0.5), (3.0, 0.5)), ("unit_square", (2.0, 2.0), (3.0, 3.0)),
    ("unit_square_ring", (0.5, 0.5), (-1.0, 0.5)), ("unit_square_ring", (0.5, 0.5), (0.5, 7.0)),
    ("box", (50.0, 40.0), (200.0, 40.0)), ("box", (50.0, 40.0), (50.0, -100.0)), ("box", (50.0, 40.0), (130.0, 100.0)),
    ("box", (0.0, 0.0), (5.0, 5.0)), ("box", (0.0, 10.0), (100.0, 10.0)), ("box", (np.nan, 40.0), (200.0, 40.0)),
    ("box", (50.0, 40.0), (np.inf, 40.0)), ("notch", (50.0, 20.0), (50.0, 200.0)), ("notch", (50.0, 60.0), (50.0, -50.0)),
    ("notch", (20.0, 50.0), (200.0, 50.0)), ("doubled", (50.0, 40.0), (200.0, 41.0)), ("doubled", (50.0, 40.0), (-200.0, 39.0)),
    ("zigzag", (0.0, 35.0), (100.0, 35.0)), ("zigzag", (47.5, 0.0), (47.5, 100.0)), ("zigzag", (-5.0, -5.0), (-1.0, 90.0)),
    ("segment", (20.0, 20.0), (80.0, 80.0)), ("segment", (20.0, 20.0), (40.0, 40.0)), ("segment", (20.0, 80.0), (80.0, 20.0)),
]

# (outline, anchor, number of angles, first angle, ray length) of the fixture's ray fans
FAN_CASES = [
    ("unit_square", (0.5, 0.5), 8, 0.0, 1000), ("unit_square_open", (0.5, 0.5), 8, 0.0, 1000),
    ("unit_square", (0.25, 0.75), 12, 0.1, 5), ("unit_square", (0.5, 0.5), 4, 0.0, 0.25),
    ("unit_square", (0.5, 0.5), 0, 0.0, 1000), ("box", (50.0, 40.0), 16, 0.0, 1000), ("box", (50.0, 40.0), 7, 0.3, 35),
    ("box", (200.0, 200.0), 9, 0.0, 50), ("notch", (50.0, 20.0), 24, 0.05, 1000), ("doubled", (30.0, 30.0), 10, 0.2, 1000),
    ("zigzag", (47.0, 35.0), 16, 0.0, 1000), ("segment", (20.0, 20.0), 16, 0.0, 100),
    ("star_3", (50.0, 50.0), 6, 0.0, 1000), ("star_8", (50.0, 50.0), 16, 0.0, 1000), ("star_21", (50.0, 50.0), 16, 0.1, 1000),
    ("star_55", (52.0, 47.0), 32, 0.0, 1000), ("star_144", (50.0, 50.0), 32, 0.02, 1000), ("star_233", (45.0, 55.0), 24, 0.0, 1000),
    ("star_300", (50.0, 50.0), 36, 0.01, 1000), ("star_300", (50.0, 50.0), 12, 0.0, 5), ("ring_9", (50.0, 50.0), 16, 0.0, 1000),
    ("ring_40", (50.0, 50.0), 16, 0.3, 1000), ("ring_150", (50.0, 50.0), 20, 0.0, 1000), ("arc_6", (50.0, 50.0), 16, 0.0, 1000),
    ("arc_30", (50.0, 50.0), 16, 0.0, 1000), ("arc_120", (50.0, 50.0), 16, 0.0, 1000), ("star_89", (0.0, 0.0), 16, 0.0, 1000),
]


def fan_angles(count, first):
    return first + np.arange(count) * (2 * np.pi / max(count, 1))


def contain_points(name, pts):
    """the fixture's points for an outline: a seeded 12 x 12 grid over its box and beyond, every vertex and every
    edge midpoint of the closed ring"""
    P = _points(pts)
    lo, hi = P.min(axis=0) - 2.0, P.max(axis=0) + 2.0
    gx, gy = np.meshgrid(np.linspace(lo[0], hi[0], 12), np.linspace(lo[1], hi[1], 12))
    mid = (P + np.roll(P, -1, axis=0)) / 2
    return np.concatenate([np.stack([gx.ravel(), gy.ravel()], 1), P, mid, [[np.nan, 50.0], [np.inf, 50.0]]])


# -------------------------------------------------------------------------------------------- lifting
SHIMS = ["geometry.LineString(points).intersection(ray) -> a Point at the restated hit, or an empty geometry",
         "geometry.Point, geos.TopologicalError -> the classes tested against; nothing raises",
         "curves.point_distance -> the pinned sqrt(dx dx + dy dy)"]


class Point(object):
    is_empty = False

    def __init__(self, xy):
        self.coords = [(float(xy[0]), float(xy[1]))]


class Empty(object):
    is_empty = True


class LineString(object):
    """an outline for the lifted code; `closed` stands for one of our Polygons"""

    def __init__(self, coords, closed=False):
        self.coords = [(float(x), float(y)) for x, y in coords]
        self.closed = closed

    def intersection(self, ray):
        _, h, edge, _ = ray_hit(ray.coords[0], ray.coords[1], self.coords, self.closed)
        return Point(h) if edge >= 0 else Empty()


def load_reference(root):
    """(get_ray_hitpoint, get_ray_intersections, get_farthest_ray_intersection) of the reference, lifted and
    shimmed"""
    POL = _sibling("make_golden_polygon")
    geometry = types.ModuleType("geometry_shim")
    geometry.LineString, geometry.Point = LineString, Point
    geos = types.ModuleType("geos_shim")
    geos.TopologicalError = type("TopologicalError", (Exception,), {})
    curves = types.ModuleType("curves_shim")
    curves.point_distance = point_distance
    ns = {"np": np, "geometry": geometry, "geos": geos, "curves": curves, "__name__": "ref_regions"}
    names = ("get_ray_hitpoint", "get_ray_intersections", "get_farthest_ray_intersection")
    POL._lift(os.path.join(root, "video", "analysis", "regions.py"), names, ns)
    return tuple(ns[n] for n in names)


def _xy(point):
    return np.array([np.nan, np.nan] if point is None else point, np.float64)


def generate(root):
    ref_hit, ref_fan, ref_far = load_reference(root)
    outs = outlines()
    data = {"shims": np.array(SHIMS), "outline_names": np.array(sorted(outs))}
    for name, (pts, closed) in outs.items():
        data["outline/%s/points" % name] = pts
        data["outline/%s/closed" % name] = np.bool_(closed)
        if closed or name.startswith(("ring_", "unit_square_ring")):
            ring = pts if closed else pts[:-1]
            cp = contain_points(name, ring)
            data["contains/%s/points" % name] = cp
            data["contains/%s/inside" % name] = contains_points([ring], cp, np.zeros(len(cp), int))
    for k, (name, anchor, far) in enumerate(RAY_CASES):
        pts, closed = outs[name]
        shape = LineString(pts, closed)
        point = ref_hit(anchor, far, shape)
        point2, dist = ref_hit(anchor, far, shape, ret_dist=True)
        assert point == point2 and point == get_ray_hitpoint(anchor, far, pts, closed), k
        assert (point is None) == bool(np.isnan(dist)), k
        data["ray/%d/hit" % k] = _xy(point)
        data["ray/%d/dist" % k] = np.float64(dist)
    for k, (name, anchor, count, first, length) in enumerate(FAN_CASES):
        pts, closed = outs[name]
        shape = LineString(pts, closed)
        angles = fan_angles(count, first)
        points = ref_fan(anchor, angles, shape, length)
        assert len(points) == count, k
        point_max, dist_max, angle_max = ref_far(anchor, angles, shape, length)
        data["fan/%d/angles" % k] = angles
        data["fan/%d/hits" % k] = np.array([_xy(p) for p in points], np.float64).reshape(-1, 2)
        data["fan/%d/farthest" % k] = np.concatenate([_xy(point_max), [dist_max, np.nan if angle_max is None
                                                                       else angle_max]]).astype(np.float64)
    return data


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("VA_REFERENCE")
    if not root or not os.path.isdir(os.path.join(root, "video", "analysis")):
        sys.stderr.write("usage: make_golden_outline.py <reference checkout> (or $VA_REFERENCE); nothing written\n")
        raise SystemExit(2)
    data = generate(root)
    np.savez_compressed(OUT, **data)
    print("wrote %s (%d arrays, %d bytes)" % (OUT, len(data), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
