"""CPU: the polygon fixture (tests/golden/polygon_v1.npz), the NumPy restatement of the fill, the distance
transform and the centre-line steps (tests/golden/make_golden_polygon.py), and the polygons' host code.  Needs
no GPU and no reference checkout.  The fill is checked against matplotlib's point-in-polygon test, the distance
transform against scipy's exact Euclidean one."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_polygon", os.path.join(ROOT, "tests", "golden", "make_golden_polygon.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(ROOT, "tests", "golden", "polygon_v1.npz"), allow_pickle=False)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_fixture_is_complete(fx):
    assert len(fx["shims"]) >= 8
    for name in G.FILL_POLYS:
        assert "position/%s" % name in fx.files and "dt/%s" % name in fx.files
        for margin in G.MARGINS:
            assert "mask/%s/%d" % (name, margin) in fx.files
    for name, _, _ in G.EST_CASES:
        assert "est/%s" % name in fx.files
    compared = [c[0] for c in G.OPT_CASES if c[3]]
    dropped = int(fx["opt_dropped"])
    # at most one compared case in four may fall below MIN_MARGIN
    assert 4 * dropped <= len(compared)
    assert len(fx["opt_kept"]) + dropped == len(compared)
    for name in fx["opt_kept"]:
        assert float(fx["opt/%s/margin" % name]) >= G.MIN_MARGIN
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "polygon_v1.npz")) < 400 * 1024


@pytest.mark.parametrize("dtype", [np.uint8, np.int32])
def test_restated_masks_reproduce_fixture(fx, dtype):
    for name, c in G.FILL_POLYS.items():
        for margin in G.MARGINS:
            mask, off = G.get_mask(c, margin, dtype)
            key = "mask/%s/%d" % (name, margin)
            assert mask.dtype == dtype
            assert np.array_equal(mask, fx[key]), key
            assert off == tuple(fx[key + "/offset"]), key


def test_restated_distance_transform_reproduces_fixture(fx):
    for name in G.FILL_POLYS:
        got = G.distance_transform(fx["mask/%s/1" % name])
        assert np.array_equal(_bits(got), _bits(fx["dt/%s" % name])), name
    for name in G.DT_EXTRA:
        got = G.distance_transform(fx["dt_extra/%s/mask" % name])
        assert np.array_equal(_bits(got), _bits(fx["dt_extra/%s" % name])), name
    # a mask without background: the DIST_MAX clamp
    assert np.all(fx["dt_extra/full"] == np.float32(G.DIST_MAX) * np.float32(1 / 65536))


def test_rowwise_distance_transform_equals_literal_passes():
    rng = np.random.default_rng(7)
    for h, w in ((1, 1), (1, 9), (9, 1), (2, 3), (13, 17), (31, 8)):
        for frac in (0.0, 0.3, 0.9, 1.0):
            m = (rng.random((h, w)) < frac).astype(np.uint8)
            assert np.array_equal(_bits(G.distance_transform(m)), _bits(G.distance_transform_literal(m))), (h, w)


def test_restated_position_and_estimates_reproduce_fixture(fx):
    from video.analysis.shapes import Polygon
    for name, c in G.FILL_POLYS.items():
        want = fx["position/%s" % name]
        assert np.array_equal(G.position(c), want), name
        assert np.array_equal(Polygon(c).position, want), name
    for name, pname, ep in G.EST_CASES:
        assert np.array_equal(G.estimate(G.FILL_POLYS[pname], ep), fx["est/%s" % name]), name


def test_restated_optimized_is_within_1e8_of_the_reference(fx):
    for name, pname, params, compared in G.OPT_CASES:
        if name not in list(fx["opt_kept"]):
            continue
        got = np.asarray(G.optimized(G.FILL_POLYS[pname], **params))
        ref = fx["opt/%s" % name]
        assert got.shape == ref.shape, name
        err = float(np.abs(got - ref).max())
        print(name, "max |restated - reference| =", err)
        assert err <= 1e-8, name


def test_rectangle_and_bounding_rect(fx):
    from video.analysis.shapes import Polygon, Rectangle
    for name, c in G.FILL_POLYS.items():
        r = Rectangle.from_points(c.max(axis=0), c.min(axis=0))
        r.buffer(1.5)
        assert np.array_equal(np.array(r.data, np.float64), fx["rect/%s" % name]), name
        p = Polygon(c)
        for margin in G.MARGINS:
            rect = p.get_bounding_rect(margin)
            assert tuple(rect[:2]) == tuple(fx["mask/%s/%d/offset" % (name, margin)])
            assert tuple(rect[[3, 2]]) == fx["mask/%s/%d" % (name, margin)].shape
    # the drop-in buffers a fresh rectangle: margins do not accumulate
    p = Polygon(G.FILL_POLYS["worm"])
    assert np.array_equal(p.get_bounding_rect(2), p.get_bounding_rect(2))
    # widths truncate: x from 0.2 to 10.1 gives a box 9 columns wide
    assert Polygon(G.FILL_POLYS["fractional"]).get_bounding_rect()[2] == 9


def test_smoothed_centerline_matches_the_reference(fx):
    from video.analysis.shapes import Polygon
    for name, kw in G.SMOOTH_CASES:
        got = np.asarray(Polygon(G.FILL_POLYS[name]).get_centerline_smoothed(
            points=fx["smooth/%s/points" % name], **kw))
        ref = fx["smooth/%s" % name]
        assert got.shape == ref.shape, name
        # host float64 code in the reference's order; only libm / FITPACK builds may differ in the last bits
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-9)


def test_get_centerline_rejects_unknown_methods():
    from video.analysis.shapes import Polygon
    with pytest.raises(ValueError):
        Polygon(G.FILL_POLYS["worm"]).get_centerline("spline")


# ---------------------------------------------------------------------- fill against matplotlib
def _seg_dist(px, py, poly):
    """distance of points to the closed polyline `poly`"""
    a = poly
    b = np.roll(poly, -1, axis=0)
    d = np.full(px.shape, np.inf)
    for (x0, y0), (x1, y1) in zip(a, b):
        vx, vy = x1 - x0, y1 - y0
        L = vx * vx + vy * vy
        t = np.zeros_like(px) if L == 0 else np.clip(((px - x0) * vx + (py - y0) * vy) / L, 0, 1)
        d = np.minimum(d, np.hypot(px - (x0 + t * vx), py - (y0 + t * vy)))
    return d


SIMPLE = ("worm", "worm_steep", "mouse", "hexagon", "star", "u_shape", "l_shape", "fractional", "negative",
          "tiny")


def _simple_polygons():
    rng = np.random.default_rng(11)
    out = [(n, G.FILL_POLYS[n]) for n in SIMPLE]
    for k in range(40):
        n = int(rng.integers(3, 24))
        t = np.sort(rng.uniform(0, 2 * np.pi, n))
        r = rng.uniform(0.3, 1.0, n) * 20
        c = rng.uniform(-5, 40, 2)
        out.append(("random%d" % k, np.stack([c[0] + r * np.cos(t) * rng.uniform(0.5, 2.0), c[1] + r * np.sin(t)], 1)))
    return out


@pytest.mark.parametrize("margin", [0, 2])
def test_fill_agrees_with_matplotlib(margin):
    """every pixel centre strictly inside the integer polygon and inside the box is set; every set pixel lies
    inside it or within 0.5 + h*2^-16 px of its boundary.  The second bound covers Bresenham's minor-axis
    error and the truncated dx's drift, which is what an edge inside its box can do; it is checked where every
    vertex lies in the box.  An edge leaving the box is first cut by clipLine, whose truncated end point moves
    the line itself: with the box (-3, -4, 11, 12) the edge (-3, -2) - (8, -4) of "negative" is drawn as
    (-3, -2) - (7, -4) and sets (5, -4), 0.537 px from the true edge.  Those cases are held to the exact
    restatement instead (tests/test_gpu_polygon.py)."""
    from matplotlib.path import Path
    unclipped = 0
    for name, c in _simple_polygons():
        mask, (ox, oy) = G.get_mask(c, margin)
        ci = np.asarray(c, np.float64).astype(np.int64).astype(np.float64)
        h, w = mask.shape
        ys, xs = np.mgrid[:h, :w]
        px, py = (xs + ox).astype(np.float64), (ys + oy).astype(np.float64)
        inside = Path(ci).contains_points(np.stack([px.ravel(), py.ravel()], 1)).reshape(h, w)
        dist = _seg_dist(px, py, ci)
        strictly = inside & (dist > 1e-9)
        assert np.all(mask[strictly] == 1), name
        if not (np.all((ci[:, 0] >= ox) & (ci[:, 0] < ox + w)) and np.all((ci[:, 1] >= oy) & (ci[:, 1] < oy + h))):
            continue
        unclipped += 1
        # the 0.5 of Bresenham's minor-axis error and the drift of the truncated dx over h rows
        bound = 0.5 + h * 2.0 ** -16
        far = (mask == 1) & ~inside
        print(name, "largest distance of a set pixel outside: %.4f (bound %.4f)"
              % (dist[far].max() if far.any() else 0.0, bound))
        assert np.all(dist[far] <= bound), name
    # with margin 0 the truncated box usually ends one column or row short of the largest vertex
    assert unclipped >= (3 if margin == 0 else 40)


def test_axis_aligned_rectangle_fills_exactly():
    rect = np.array([[2, 3], [9, 3], [9, 7], [2, 7]])
    for box in ((0, 0, 12, 10), (2, 3, 8, 5), (-1, -2, 15, 12)):
        mask = G.fill_poly(rect, box)
        want = np.zeros_like(mask)
        want[3 - box[1]:8 - box[1], 2 - box[0]:10 - box[0]] = 1
        assert np.array_equal(mask, want), box


def test_fill_clips_vertices_outside_the_box():
    # truncation puts vertices outside the box: the lines are clipped, nothing is written outside
    mask, off = G.get_mask(G.FILL_POLYS["negative"], 0)
    assert mask.shape == (12, 11) and off == (-3, -4)
    assert mask.any()
    tiny = G.fill_poly(np.array([[-5, -5], [40, -5], [40, 40], [-5, 40]]), (0, 0, 4, 3))
    assert np.array_equal(tiny, np.ones((3, 4), np.uint8))


# ------------------------------------------------------------------ distance transform against scipy
def _blobs(rng, h, w):
    from scipy import ndimage
    m = rng.random((h, w)) < 0.5
    for _ in range(3):
        m = ndimage.uniform_filter(m.astype(float), 5) > 0.5
    return m.astype(np.uint8)


def test_distance_transform_within_chamfer_bounds_of_edt(fx):
    """the (1, 1.4, 2.1969) chamfer's straight-line distance over the Euclidean one spans 0.9825 (direction
    (2, 1)) to 1.0192 (slope 0.1969), plus the weights' 2^-16 rounding: every foreground ratio lies in
    [0.98, 1.02] on masks with at least one zero pixel"""
    from scipy import ndimage
    rng = np.random.default_rng(3)
    masks = [_blobs(rng, 64, 96) for _ in range(6)]
    one_zero = np.ones((81, 81), np.uint8)
    one_zero[40, 40] = 0
    masks.append(one_zero)
    masks += [fx["mask/%s/1" % n] for n in G.FILL_POLYS]
    lo, hi = np.inf, -np.inf
    for m in masks:
        if m.all():
            continue
        d = G.distance_transform(m).astype(np.float64)
        e = ndimage.distance_transform_edt(m)
        fg = m != 0
        if not fg.any():
            continue
        r = d[fg] / e[fg]
        lo, hi = min(lo, r.min()), max(hi, r.max())
    print("chamfer / edt ratios: [%.5f, %.5f]" % (lo, hi))
    assert 0.98 <= lo and hi <= 1.02
