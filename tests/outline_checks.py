"""Shared by tests/test_outline_public_host.py (CPU, the ops replaced by the restatement) and tests/test_gpu_outline.py
(the real ops): the generator's restatement, bit-pattern comparison, and the walk through the whole fixture
outline_v1.npz by way of the public functions of video.analysis.regions and video.analysis.shapes.  No test lives
here, and nothing here imports torch or loads the library."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_outline", os.path.join(ROOT, "tests", "golden", "make_golden_outline.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()


def load_fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "outline_v1.npz"), allow_pickle=False)


def bits(a):
    """float64 as uint64, so that -0.0 and the NaN pattern count"""
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def same_bits(got, want, what=None):
    g, w = np.asarray(got), np.asarray(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if w.dtype == np.float64:
        assert g.dtype == np.float64, (what, g.dtype)
        assert np.array_equal(bits(g), bits(w)), (what, g, w)
    else:
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, g, w)


def same_results(got, want, what=None):
    """the four arrays of ops.ray_hits / G.ray_hits"""
    assert len(got) == len(want) == 4, what
    want = (np.asarray(want[0], np.float64), np.asarray(want[1], np.float64), np.asarray(want[2], np.int32),
            np.asarray(want[3], np.int32))
    for name, g, w in zip(("t", "hits", "edge", "count"), got, want):
        same_bits(g, w, (what, name))


def point_bits(p):
    return bits(np.array([np.nan, np.nan] if p is None else p, np.float64))


class Coords(object):
    """an outline argument of the third form: any object with .coords"""

    def __init__(self, pts):
        self.coords = [(float(x), float(y)) for x, y in pts]


def outline_forms(pts, closed):
    """the public outline arguments that stand for (pts, closed)"""
    from video.analysis.shapes import Polygon
    if closed:
        return [Polygon(pts)]
    return [pts, pts.tolist(), Coords(pts)]


def check_fixture_rays(fx):
    """every ray/* and fan/* entry through regions.get_ray_hitpoint, get_ray_intersections and
    get_farthest_ray_intersection, in every argument form; returns the number of public calls made"""
    from video.analysis import regions
    outs = G.outlines()
    calls = 0
    for k, (name, anchor, far) in enumerate(G.RAY_CASES):
        pts, closed = outs[name]
        want_hit, want_dist = fx["ray/%d/hit" % k], fx["ray/%d/dist" % k]
        for shape in outline_forms(pts, closed):
            point = regions.get_ray_hitpoint(anchor, far, shape)
            point2, dist = regions.get_ray_hitpoint(anchor, far, shape, ret_dist=True)
            calls += 2
            assert point == point2, k
            if np.isnan(want_hit).any():
                assert point is None and isinstance(dist, float) and np.isnan(dist), k
            else:
                assert isinstance(point, tuple) and all(type(v) is float for v in point), k
                assert type(dist) is float, k
            assert np.array_equal(point_bits(point), bits(want_hit)), (k, point, want_hit)
            assert np.array_equal(bits(dist), bits(want_dist)), (k, dist, want_dist)
    for k, (name, anchor, count, first, length) in enumerate(G.FAN_CASES):
        pts, closed = outs[name]
        angles = fx["fan/%d/angles" % k]
        want_hits, want_far = fx["fan/%d/hits" % k], fx["fan/%d/farthest" % k]
        for shape in outline_forms(pts, closed)[:2]:
            points = regions.get_ray_intersections(anchor, angles, shape, length)
            best = regions.get_farthest_ray_intersection(anchor, angles, shape, length)
            calls += 2
            assert isinstance(points, list) and len(points) == count, k
            got = np.array([[np.nan, np.nan] if p is None else p for p in points], np.float64).reshape(-1, 2)
            assert np.array_equal(bits(got), bits(want_hits)), k
            if best[0] is None:
                assert best == (None, 0, None), k
            got_far = np.concatenate([[np.nan, np.nan] if best[0] is None else best[0],
                                      [best[1], np.nan if best[2] is None else best[2]]]).astype(np.float64)
            assert np.array_equal(bits(got_far), bits(want_far)), (k, best, want_far)
    return calls


def fixture_rings(fx):
    """name -> (ring, points, inside) of every contains/* entry"""
    outs = G.outlines()
    rings = {}
    for name in sorted(k.split("/")[1] for k in fx.files if k.startswith("contains/") and k.endswith("/inside")):
        pts, closed = outs[name]
        rings[name] = (pts if closed else pts[:-1], fx["contains/%s/points" % name], fx["contains/%s/inside" % name])
    return rings


def check_fixture_containment(fx):
    """every contains/* entry through Polygon.contains_points, Polygon.contains and shapes.contains_points"""
    from video.analysis import shapes
    rings = fixture_rings(fx)
    assert len(rings) >= 20
    for name, (ring, cp, want) in rings.items():
        poly = shapes.Polygon(ring)
        got = poly.contains_points(cp)
        assert got.dtype == np.bool_ and np.array_equal(got, want), name
        for j in (0, len(cp) // 2, len(cp) - 1, int(np.flatnonzero(want)[0])):
            one = poly.contains(cp[j])
            assert type(one) is bool and one == bool(want[j]), (name, j)
    names = sorted(rings)
    polys = [shapes.Polygon(rings[n][0]) if k % 2 else rings[n][0] for k, n in enumerate(names)]
    pts = np.concatenate([rings[n][1] for n in names])
    index = np.repeat(np.arange(len(names)), [len(rings[n][1]) for n in names])
    assert len(pts) == 5504
    got = shapes.contains_points(polys, pts, index)
    assert np.array_equal(got, np.concatenate([rings[n][2] for n in names]))
