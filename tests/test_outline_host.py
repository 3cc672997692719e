"""CPU: the pinned outline queries ("Outline queries") -- the fixture outline_v1.npz is complete and
reproduced by the NumPy restatement of tests/golden/make_golden_outline.py, the restatement has the known answers of
the unit square and keeps the first of equal maxima, and its containment equals matplotlib's on seeded simple rings.
Reads the npz and the generator's restatement only."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_outline", os.path.join(ROOT, "tests", "golden", "make_golden_outline.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()
SQUARE = np.array(G.SQUARE)


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(ROOT, "tests", "golden", "outline_v1.npz"), allow_pickle=False)


def _point(p):
    return np.array([np.nan, np.nan] if p is None else p, np.float64)


# ------------------------------------------------------------------------------- fixture and restatement
def test_fixture_is_complete_and_small(fx):
    outs = G.outlines()
    assert sorted(outs) == fx["outline_names"].tolist() and 24 <= len(outs) <= 48
    assert max(len(p) for p, _ in outs.values()) <= 301
    assert list(fx["shims"]) == G.SHIMS
    keys = {"shims", "outline_names"}
    for name, (pts, closed) in outs.items():
        keys |= {"outline/%s/points" % name, "outline/%s/closed" % name}
        assert np.array_equal(fx["outline/%s/points" % name], pts) and bool(fx["outline/%s/closed" % name]) == closed
    for k in range(len(G.RAY_CASES)):
        keys |= {"ray/%d/hit" % k, "ray/%d/dist" % k}
    for k in range(len(G.FAN_CASES)):
        keys |= {"fan/%d/angles" % k, "fan/%d/hits" % k, "fan/%d/farthest" % k}
    contained = [k.split("/")[1] for k in fx.files if k.startswith("contains/") and k.endswith("/inside")]
    assert len(contained) >= 20
    for name in contained:
        keys |= {"contains/%s/points" % name, "contains/%s/inside" % name}
    assert keys == set(fx.files)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "outline_v1.npz")) < 400 * 1024


def test_restatement_reproduces_the_fixture(fx):
    outs = G.outlines()
    for k, (name, anchor, far) in enumerate(G.RAY_CASES):
        pts, closed = outs[name]
        point, dist = G.get_ray_hitpoint(anchor, far, pts, closed, ret_dist=True)
        assert np.array_equal(_point(point), fx["ray/%d/hit" % k], equal_nan=True), k
        assert np.array_equal(np.float64(dist), fx["ray/%d/dist" % k], equal_nan=True), k
    hit_any = missed_any = False
    for k, (name, anchor, count, first, length) in enumerate(G.FAN_CASES):
        pts, closed = outs[name]
        angles = G.fan_angles(count, first)
        assert np.array_equal(angles, fx["fan/%d/angles" % k])
        points, best = G.get_farthest_ray_intersection(anchor, angles, pts, closed, length)
        hits = np.array([_point(p) for p in points], np.float64).reshape(-1, 2)
        assert np.array_equal(hits, fx["fan/%d/hits" % k], equal_nan=True), k
        want = np.concatenate([_point(best[0]), [best[1], np.nan if best[2] is None else best[2]]])
        assert np.array_equal(want, fx["fan/%d/farthest" % k], equal_nan=True), k
        hit_any |= bool(np.isfinite(hits).any())
        missed_any |= bool(np.isnan(hits).any())
    assert hit_any and missed_any
    for name in (k.split("/")[1] for k in fx.files if k.startswith("contains/") and k.endswith("/inside")):
        pts, closed = outs[name]
        ring = pts if closed else pts[:-1]
        cp = fx["contains/%s/points" % name]
        assert np.array_equal(cp, G.contain_points(name, ring), equal_nan=True)
        want = fx["contains/%s/inside" % name]
        assert np.array_equal(G.contains_points([ring], cp, np.zeros(len(cp), int)), want), name
        assert want.dtype == np.bool_ and want.any() and not want.all(), name


def test_known_answers_of_the_unit_square():
    t, h, edge, count = G.ray_hit((0.5, 0.5), (2.0, 0.5), SQUARE, True)
    assert (t, h, edge, count) == (1.0 / 3.0, (1.0, 0.5), 1, 1)
    assert G.get_ray_hitpoint((0.5, 0.5), (2.0, 0.5), SQUARE, True, ret_dist=True) == ((1.0, 0.5), 0.5)
    # the open array of the four points has no edge from (0, 1) back to (0, 0)
    assert G.ray_hit((0.5, 0.5), (-1.0, 0.5), SQUARE, False)[2:] == (-1, 0)
    assert G.get_ray_hitpoint((0.5, 0.5), (-1.0, 0.5), SQUARE, False) is None
    assert G.ray_hit((0.5, 0.5), (-1.0, 0.5), SQUARE, True)[1:] == ((0.0, 0.5), 3, 1)
    assert G.ray_hit((0.5, 0.5), (-1.0, 0.5), np.concatenate([SQUARE, SQUARE[:1]]), False)[1:] == ((0.0, 0.5), 3, 1)
    # through the corner (1, 1): edges 1 and 2 both report it, the lower index wins
    t, h, edge, count = G.ray_hit((0.5, 0.5), (1.5, 1.5), SQUARE, True)
    assert (t, h, edge, count) == (0.5, (1.0, 1.0), 1, 2)
    # lying on edge 0: the edge itself is parallel and never counts, its end vertices do through edges 3 and 1
    t, hit = G.ray_edges((-1.0, 0.0), (2.0, 0.0), SQUARE, True)
    assert hit.tolist() == [False, True, False, True]
    assert t[3] == 1.0 / 3.0 and t[1] == 2.0 / 3.0
    assert G.ray_hit((-1.0, 0.0), (2.0, 0.0), SQUARE, True)[1:] == ((0.0, 0.0), 3, 2)
    # a zero-length ray hits nothing, not even from a vertex; neither does a NaN
    for p in ((0.5, 0.5), (1.0, 1.0), (0.0, 0.5)):
        assert G.ray_hit(p, p, SQUARE, True)[2:] == (-1, 0)
    assert G.ray_hit((np.nan, 0.5), (2.0, 0.5), SQUARE, True)[2:] == (-1, 0)
    assert G.ray_hit((0.5, 0.5), (2.0, np.nan), SQUARE, True)[2:] == (-1, 0)
    # t = 0 and t = 1 exactly
    assert G.ray_hit((1.0, 0.5), (3.0, 0.5), SQUARE, True)[:3] == (0.0, (1.0, 0.5), 1)
    assert G.ray_hit((0.5, 0.5), (1.0, 0.5), SQUARE, True)[:3] == (1.0, (1.0, 0.5), 1)
    # no points, one point, a doubled point
    assert G.ray_hit((0.5, 0.5), (2.0, 0.5), np.zeros((0, 2)), True)[2:] == (-1, 0)
    assert G.ray_hit((0.5, 0.5), (2.0, 0.5), [(1.0, 0.5)], True)[2:] == (-1, 0)
    assert G.ray_hit((0.5, 0.5), (2.0, 0.5), np.repeat(SQUARE, 2, axis=0), True)[1:] == ((1.0, 0.5), 3, 1)


def test_the_pair_order_does_not_depend_on_the_edge_order():
    """the smallest (t, i) found from any split of the edges into parts is the one of the whole"""
    rng = np.random.default_rng(3)
    pts = G.star_ring(rng, 97, step=0.5)
    for k in range(40):
        a, f = rng.uniform(40, 60, 2).round(), rng.uniform(-50, 150, 2).round()
        t, hit = G.ray_edges(a, f, pts, True)
        whole = G.ray_hit(a, f, pts, True)
        best = None
        for part in np.array_split(rng.permutation(len(t)), 7):
            for i in part[hit[part]]:
                if best is None or (t[i], i) < best:
                    best = (t[i], int(i))
        assert (whole[2] < 0 and best is None) or (whole[0], whole[2]) == best
        assert whole[3] == hit.sum()


def test_containment_equals_matplotlib_on_simple_rings():
    mpath = pytest.importorskip("matplotlib.path")
    rng = np.random.default_rng(4)
    compared = 0
    for k in range(60):
        ring = G.star_ring(rng, int(rng.integers(3, 40)), step=0.5)
        points = rng.uniform(5, 95, (50, 2))
        want = mpath.Path(np.concatenate([ring, ring[:1]]), closed=True).contains_points(points)
        got = G.contains_points([ring], points, np.zeros(len(points), int))
        assert np.array_equal(got, want), k
        compared += len(points)
    assert compared == 3000


def test_vertices_and_edge_midpoints_of_integer_rings_are_outside():
    rng = np.random.default_rng(5)
    for k in range(20):
        ring = G.star_ring(rng, int(rng.integers(3, 30)), step=2.0)          # even: the midpoints are whole too
        mid = (ring + np.roll(ring, -1, axis=0)) / 2
        both = np.concatenate([ring, mid])
        assert not G.contains_points([ring], both, np.zeros(len(both), int)).any(), k
    assert G.contains(SQUARE, (0.5, 0.5)) and not G.contains(SQUARE, (1.5, 0.5))
    assert not G.contains(SQUARE, (1.0, 0.5)) and not G.contains(SQUARE, (1.0, 1.0))
    assert not G.contains(SQUARE[:2], (0.5, 0.0)) and not G.contains(np.zeros((0, 2)), (0.0, 0.0))
    assert not G.contains(SQUARE, (np.nan, 0.5)) and not G.contains(SQUARE, (0.5, np.inf))
    assert not G.contains(SQUARE, (-np.inf, 0.5))


def test_farthest_ray_keeps_the_first_of_equal_maxima():
    """(0.5, 0.5) in the unit square is hit at distance 0.5 exactly towards 0 and towards pi"""
    far = (0.5 + 1000 * np.cos(np.pi), 0.5 + 1000 * np.sin(np.pi))
    assert G.get_ray_hitpoint((0.5, 0.5), far, SQUARE, True, ret_dist=True)[1] == 0.5
    assert G.get_ray_hitpoint((0.5, 0.5), (1000.5, 0.5), SQUARE, True, ret_dist=True)[1] == 0.5
    assert G.get_farthest_ray_intersection((0.5, 0.5), [0.0, np.pi], SQUARE, True)[1][1:] == (0.5, 0.0)
    assert G.get_farthest_ray_intersection((0.5, 0.5), [np.pi, 0.0], SQUARE, True)[1][1:] == (0.5, np.pi)
    assert G.get_farthest_ray_intersection((0.5, 0.5), [0.0, np.pi, np.pi / 4], SQUARE, True)[1][2] == np.pi / 4
    # no hit at all, and no angle at all: the reference's start values
    assert G.get_farthest_ray_intersection((0.5, 0.5), [0.0, 1.0], SQUARE, True, 0.1) == ([None, None], (None, 0, None))
    assert G.get_farthest_ray_intersection((0.5, 0.5), [], SQUARE, True) == ([], (None, 0, None))
