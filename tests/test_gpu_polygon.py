"""GPU: polygon masks (va_fill_poly), distance transforms (va_distance_transform_l2_5) and the centre lines of
video.analysis.shapes.Polygon against the NumPy restatement of tests/golden/make_golden_polygon.py and the
reference-run fixture polygon_v1.npz.  Reads the npz and the generator's restatement only."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

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
    from video import _hip
    _hip.lib()
    return np.load(os.path.join(ROOT, "tests", "golden", "polygon_v1.npz"), allow_pickle=False)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _random_cases(seed, count, span=40.0):
    """seeded random polygons with boxes of mixed sizes: the polygon's own box with a random margin, or a random
    box that cuts it"""
    rng = np.random.default_rng(seed)
    contours, boxes = [], []
    for k in range(count):
        c = G.random_polygon(rng, span=float(rng.choice([6.0, span, 3 * span])))
        if rng.random() < 0.3:
            c = c * rng.uniform(-1.5, 1.5)
        ci = c.astype(np.int64)
        if rng.random() < 0.7:
            box = tuple(int(v) for v in G.bounding_rect(c, int(rng.integers(0, 4))))
        else:
            lo = ci.min(axis=0) - 3
            box = (int(rng.integers(lo[0], lo[0] + 20)), int(rng.integers(lo[1], lo[1] + 20)),
                   int(rng.integers(0, 50)), int(rng.integers(0, 50)))
        contours.append(ci)
        boxes.append(box)
    return contours, boxes


# ----------------------------------------------------------------------------------------------- masks
@pytest.mark.parametrize("dtype", [np.uint8, np.int32])
def test_masks_equal_fixture(fx, dtype):
    from video.analysis.shapes import Polygon
    for name, c in G.FILL_POLYS.items():
        for margin in G.MARGINS:
            mask, off = Polygon(c).get_mask(margin, dtype, ret_offset=True)
            key = "mask/%s/%d" % (name, margin)
            assert mask.dtype == dtype, key
            assert np.array_equal(mask, fx[key]), key
            assert tuple(off) == tuple(fx[key + "/offset"]), key


@pytest.mark.parametrize("dtype", [np.uint8, np.int32])
def test_batched_masks_equal_per_item(fx, dtype):
    from video.analysis.shapes import Polygon, get_masks
    polys = [Polygon(c) for c in G.FILL_POLYS.values()]
    for margin in (0, 3):
        masks, offs = get_masks(polys, margin, dtype, ret_offset=True)
        for p, m, o in zip(polys, masks, offs):
            one, o1 = p.get_mask(margin, dtype, ret_offset=True)
            assert m.dtype == dtype and np.array_equal(m, one) and tuple(o) == tuple(o1)


@pytest.mark.parametrize("dtype", [np.uint8, np.int32])
def test_random_polygons_equal_restatement(dtype):
    from video import ops
    contours, boxes = _random_cases(1234, 300)
    got = ops.fill_polys(contours, boxes, dtype)
    for k, (c, b) in enumerate(zip(contours, boxes)):
        want = G.fill_poly(c, b, dtype)
        assert got[k].dtype == dtype and got[k].shape == want.shape, k
        assert np.array_equal(got[k], want), (k, c.tolist(), b)
    # one launch per polygon gives the same bytes
    for k in range(0, 300, 37):
        assert np.array_equal(ops.fill_polys([contours[k]], [boxes[k]], dtype)[0], got[k])


def test_large_and_degenerate_polygons_equal_restatement():
    from video import ops
    rng = np.random.default_rng(5)
    t = np.linspace(0, 2 * np.pi, 1000, endpoint=False)
    big = np.stack([700 + 650 * np.cos(t) * (1 + 0.1 * np.sin(7 * t)), 400 + 380 * np.sin(t)], 1).astype(np.int64)
    cases = [(big, (0, 0, 1400, 800)), (big, (50, 20, 1300, 700)),
             (np.array([[3, 4]]), (0, 0, 8, 8)),                                   # one vertex: one pixel
             (np.array([[1, 4], [12, 4], [6, 4]]), (0, 0, 14, 9)),                # one row
             (np.array([[3, 1], [3, 9], [3, 5]]), (0, 0, 6, 12)),                 # one column
             (np.array([[0, 0], [5, 5], [9, 2]]), (0, 0, 0, 7)),                  # empty box
             (np.array([[-900000, -5], [900000, 3], [0, 900000]]), (-10, -10, 40, 30)),   # far vertices, clipped
             (rng.integers(-30, 60, (1024, 2)), (0, 0, 40, 40))]                  # 1024 vertices, self-crossing
    got = ops.fill_polys([c for c, _ in cases], [b for _, b in cases])
    for k, (c, b) in enumerate(cases):
        assert np.array_equal(got[k], G.fill_poly(c, b)), k
    # an axis-aligned integer rectangle fills exactly, both ends included
    rect = np.array([[2, 3], [9, 3], [9, 7], [2, 7]])
    for box in ((0, 0, 12, 10), (2, 3, 8, 5), (-1, -2, 15, 12)):
        want = np.zeros((box[3], box[2]), np.uint8)
        want[3 - box[1]:8 - box[1], 2 - box[0]:10 - box[0]] = 1
        assert np.array_equal(ops.fill_polys([rect], [box])[0], want), box


# -------------------------------------------------------------------------------- distance transform
def test_distance_transform_equals_fixture(fx):
    from video import ops
    masks = [fx["mask/%s/1" % n] for n in G.FILL_POLYS] + [fx["dt_extra/%s/mask" % n] for n in G.DT_EXTRA]
    wants = [fx["dt/%s" % n] for n in G.FILL_POLYS] + [fx["dt_extra/%s" % n] for n in G.DT_EXTRA]
    got = ops.distance_transform(masks)
    for k, (g, w) in enumerate(zip(got, wants)):
        assert g.dtype == np.float32 and np.array_equal(_bits(g), _bits(w)), k


def test_distance_transform_random_masks_equal_restatement():
    from video import ops
    rng = np.random.default_rng(9)
    shapes = [(1, 1), (1, 300), (300, 1), (2, 2), (17, 255), (33, 256), (40, 257), (5, 1000), (120, 700),
              (64, 4096), (600, 31)]
    masks = []
    for h, w in shapes:
        for frac in (0.5, 0.97):
            masks.append(G.blob_mask(rng, h, w) if frac == 0.5 else (rng.random((h, w)) < frac).astype(np.uint8))
    masks.append(np.ones((50, 60), np.uint8))
    masks.append(np.full((7, 9), 3, np.uint8))          # every non-zero value is foreground
    got = ops.distance_transform(masks)
    for k, m in enumerate(masks):
        assert np.array_equal(_bits(got[k]), _bits(G.distance_transform(m))), (k, m.shape)
    for k in (0, 5, 13, len(masks) - 1):
        assert np.array_equal(_bits(ops.distance_transform([masks[k]])[0]), _bits(got[k]))


# -------------------------------------------------------------------------------------- centre lines
def _est_cases():
    for name, pname, ep in G.EST_CASES:
        yield name, G.FILL_POLYS[pname], ep


def test_estimates_equal_fixture(fx):
    from video.analysis.shapes import Polygon
    for name, c, ep in _est_cases():
        got = Polygon(c).get_centerline_estimate(ep)
        assert got.dtype == np.int64 and np.array_equal(got, fx["est/%s" % name]), name


def test_padded_batch_of_estimates_equals_per_item(fx):
    from video.analysis.shapes import Polygon, get_centerline_estimates
    polys, eps, wants = [], [], []
    for name, c, ep in _est_cases():
        polys.append(Polygon(c))
        eps.append(ep)
        wants.append(fx["est/%s" % name])
    rng = np.random.default_rng(21)
    for k in range(24):                                  # mixed box sizes, so several stacks and padding
        c = G.worm(length=float(rng.uniform(20, 160)), width=float(rng.uniform(3, 9)),
                   bend=float(rng.uniform(0, 20)), x0=float(rng.uniform(-5, 30)), y0=float(rng.uniform(10, 40)),
                   phase=float(rng.uniform(0, 3)))
        polys.append(Polygon(c))
        eps.append(None if k % 3 else G.estimate(c)[[0, 5]])
        wants.append(G.estimate(c, eps[-1]))
    got = get_centerline_estimates(polys, eps)
    for k, (g, w) in enumerate(zip(got, wants)):
        assert np.array_equal(g, w), k
        assert np.array_equal(g, polys[k].get_centerline_estimate(eps[k])), k
    assert all(np.array_equal(a, b) for a, b in zip(get_centerline_estimates(polys[:5]),
                                                    [p.get_centerline_estimate() for p in polys[:5]]))


def test_end_point_off_the_mask_raises():
    from video.analysis.shapes import Polygon
    p = Polygon(G.FILL_POLYS["worm"])
    with pytest.raises(ValueError):
        p.get_centerline_estimate(np.array([[14, 21], [90, 14]]))       # (90, 14) lies outside the worm


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_optimized_is_bit_exact_and_within_1e8_of_the_reference(fx):
    from video.analysis.shapes import Polygon
    kept = list(fx["opt_kept"])
    for name, pname, params, compared in G.OPT_CASES:
        c = G.FILL_POLYS[pname]
        got = np.asarray(Polygon(c).get_centerline_optimized(**params))
        want = np.asarray(G.optimized(c, **params))
        assert got.shape == want.shape and np.array_equal(_bits64(got), _bits64(want)), name
        if compared and name in kept:
            err = float(np.abs(got - fx["opt/%s" % name]).max())
            print(name, "max |gpu - reference| =", err)
            assert err <= 1e-8, name


def test_default_centerline_is_the_smoothed_optimized_one():
    from video.analysis.shapes import Polygon
    c = G.FILL_POLYS["worm"]
    p = Polygon(c)
    got = np.asarray(p.get_centerline())
    want = np.asarray(p.get_centerline_smoothed(points=np.asarray(G.optimized(c, spacing=10))))
    assert np.array_equal(_bits64(got), _bits64(want))
    assert np.array_equal(np.asarray(p.get_centerline("estimate")), G.estimate(c))


def test_skeleton_points():
    from video.analysis.image import mask_thinning
    from video.analysis.shapes import Polygon
    p = Polygon(G.FILL_POLYS["worm"])
    mask, off = G.get_mask(p.contour, 5)
    skel = mask_thinning(mask)
    y, x = np.nonzero(skel)
    assert np.array_equal(p.get_skeleton_points(), np.c_[x, y] + off)
    assert np.array_equal(p.get_skeleton(), mask_thinning(G.get_mask(p.contour, 0)[0]))


# -------------------------------------------------------------------------------- limits and streams
def test_error_codes_and_limits():
    from video import _hip, ops
    from video._hip import DeviceBuffer
    L = _hip.lib()
    tri = np.array([[0, 0], [5, 0], [0, 5]], np.int32)
    assert L.va_fill_poly(None, None, 0, None, None, 0, -1, 1, None, None, None) == -22
    assert L.va_fill_poly(None, None, 0, None, None, 0, 1, 2, None, None, None) == -22
    assert L.va_fill_poly(None, None, 0, None, None, 0, 1, 1, None, None, None) == -22
    assert L.va_fill_poly(None, None, 0, None, None, 0, 0, 1, None, None, None) == 0
    assert L.va_distance_transform_l2_5(None, None, None, 0, 1, 5000, None, None, None) == -22
    assert L.va_distance_transform_l2_5(None, None, None, 0, -1, 8, None, None, None) == -22

    # per-polygon status: too many vertices, a box side too large, an offset beyond the buffer, a far vertex
    verts = np.zeros((1100, 2), np.int32)
    verts[:3] = tri
    vert_off = np.array([0, 3, 3 + 1025, 3 + 1025 + 3, 3 + 1025 + 3 + 3, 1037], np.int64)
    verts[1031:1034] = tri
    verts[1034:1037] = [[0, 0], [(1 << 20) + 1, 0], [0, 3]]
    boxes = np.array([[0, 0, 6, 6], [0, 0, 6, 6], [0, 0, 16385, 1], [0, 0, 6, 6], [0, 0, 6, 6]], np.int32)
    out_off = np.array([0, 36, 72, 0, 0], np.int64)
    out_off[3] = 10 ** 6
    bufs = [DeviceBuffer.from_array(a) for a in (verts, vert_off, boxes, out_off)]
    out, st = DeviceBuffer(200), DeviceBuffer(5 * 4)
    assert L.va_fill_poly(bufs[0].ptr, bufs[1].ptr, len(verts), bufs[2].ptr, bufs[3].ptr, 200, 5, 1, out.ptr,
                          st.ptr, None) == 0
    assert st.download((5,), np.int32).tolist() == [0, -34, -34, -34, -34]
    assert np.array_equal(out.download((36,), np.uint8).reshape(6, 6), G.fill_poly(tri, (0, 0, 6, 6)))

    shapes = np.array([[4, 4], [2, 9], [16385, 1]], np.int32)
    offs = np.array([0, 16, 0], np.int64)
    mb = DeviceBuffer.from_array(np.ones(64, np.uint8))
    sb, ob, db, st2 = DeviceBuffer.from_array(shapes), DeviceBuffer.from_array(offs), DeviceBuffer(256), \
        DeviceBuffer(12)
    assert L.va_distance_transform_l2_5(mb.ptr, sb.ptr, ob.ptr, 64, 3, 8, db.ptr, st2.ptr, None) == 0
    assert st2.download((3,), np.int32).tolist() == [0, -34, -34]          # 9 columns > max_w 8; too tall

    with pytest.raises(ValueError):
        ops.fill_polys([np.zeros((1025, 2), np.int64)], [(0, 0, 4, 4)])
    with pytest.raises(ValueError):
        ops.fill_polys([tri], [(0, 0, -1, 4)])
    with pytest.raises(TypeError):
        ops.fill_polys([tri.astype(np.float64)], [(0, 0, 4, 4)])
    with pytest.raises(ValueError):
        ops.distance_transform([np.ones((3, 4097), np.uint8)])
    assert ops.fill_polys([], []) == [] and ops.distance_transform([]) == []


def test_created_stream_back_to_back():
    from video import _hip, ops
    L = _hip.lib()
    s = C.c_void_p()
    assert L.va_stream_create(C.byref(s)) == 0
    try:
        for seed in range(4):
            contours, boxes = _random_cases(100 + seed, 40)
            masks = ops.fill_polys(contours, boxes, np.uint8, stream=s.value)
            dts = ops.distance_transform(masks, stream=s.value)
            for c, b, m, d in zip(contours, boxes, masks, dts):
                want = G.fill_poly(c, b)
                assert np.array_equal(m, want)
                assert np.array_equal(_bits(d), _bits(G.distance_transform(want)))
    finally:
        L.va_stream_destroy(s.value)
