"""CPU: the host side of the batched centre lines -- the new ops and shape functions exist and fail loudly without
a device, list arguments are checked before anything reaches the GPU, and the spline helper that
Polygon.get_centerline_smoothed and get_centerlines_smoothed share returns what the method returned."""
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


def _needs_device(fn):
    """fn() reaches the GPU: without one it raises HipUnavailableError and nothing else; with one it runs"""
    from video import _hip
    if _hip.gpu_available():
        return fn()
    with pytest.raises(_hip.HipUnavailableError):
        fn()


def _polygons(names=("worm", "mouse", "hexagon")):
    from video.analysis.shapes import Polygon
    return [Polygon(G.FILL_POLYS[n]) for n in names]


def test_new_entry_points_are_bound():
    from video import _hip, ops
    for name in ("va_potential_gradients_ragged", "va_active_contour_ragged"):
        assert name in _hip.SIGNATURES, name
        assert hasattr(_hip.load_library(), name), name
    header = open(os.path.join(ROOT, "include", "videoanalysis_hip.h")).read()
    assert "#define VA_GRAD_RESIDENT_MAX_PIXELS %d\n" % ops.GRAD_RESIDENT_MAX_PIXELS in header
    assert ops.GRAD_RESIDENT_MAX_PIXELS * 8 <= 64 * 1024        # two float32 planes in LDS without an opt-in


def test_ops_fail_loudly_without_a_device():
    from video import ops
    items = [np.zeros((5, 7), np.float32), np.zeros((3, 4), np.float32)]
    _needs_device(lambda: [b.free() for b in ops.potential_gradients_ragged(items, 1.0)[:2]])
    _needs_device(lambda: [b.free() for b in ops.potential_gradients_ragged([])[:2]])
    contours = [np.array([[1, 1], [8, 1], [8, 6], [1, 6]]), np.array([[0, 0], [4, 0], [2, 5]])]
    boxes = [(0, 0, 10, 8), (-1, -1, 7, 8)]
    _needs_device(lambda: [b.free() for b in ops.centerline_gradients(contours, boxes)[:2]])

    class Planes(object):                # active_contour_ragged asks the library before it touches the planes
        ptr = 0
    shapes, offsets = np.array([[5, 7], [3, 4]], np.int32), np.array([0, 35], np.int64)
    pts = np.zeros((1, 4, 2))
    _needs_device(lambda: ops.active_contour_ragged(Planes(), Planes(), shapes, offsets, pts[:0], [], [], np.zeros(1),
                                                    [], None, None, 0.01, 0.01, 5))


def test_shape_functions_fail_loudly_without_a_device():
    from video.analysis import shapes
    polys = _polygons()
    _needs_device(lambda: shapes.get_centerlines_optimized(polys, spacing=5, max_iterations=5))
    _needs_device(lambda: shapes.get_centerlines_smoothed(polys[:1], spacing=5, skip_length=10, max_iterations=5))
    for method in ("smoothed", "optimized", "estimate"):
        _needs_device(lambda: shapes.get_centerlines(polys[:1], method=method))
    _needs_device(lambda: shapes.get_centerlines_optimized([]))
    with pytest.raises(ValueError):
        shapes.get_centerlines(polys, method="spline")


def test_ragged_potentials_fail_loudly_without_a_device():
    from video.analysis.active_contour import ActiveContour
    ac = ActiveContour(blur_radius=1)
    _needs_device(lambda: ac.set_potential([np.zeros((5, 7), np.float32), np.zeros((6, 4), np.float32)]))


def test_mismatched_lists_raise_value_error():
    from video import ops
    from video.analysis import shapes
    from video.analysis.active_contour import ActiveContour
    polys = _polygons()
    with pytest.raises(ValueError):
        shapes.get_centerlines_optimized(polys, endpoints=[None, None])
    with pytest.raises(ValueError):
        shapes.get_centerlines_smoothed(polys, endpoints=[None] * 4)
    with pytest.raises(ValueError):
        shapes.get_centerlines(polys, method="optimized", endpoints=[])
    contours = [np.array([[1, 1], [8, 1], [8, 6]]), np.array([[0, 0], [4, 0], [2, 5]])]
    with pytest.raises(ValueError):
        ops.centerline_gradients(contours, [(0, 0, 10, 8)])
    with pytest.raises(TypeError):
        ops.centerline_gradients([c.astype(np.float64) for c in contours], [(0, 0, 10, 8)] * 2)
    with pytest.raises(ValueError):
        ops.centerline_gradients(contours, [(0, 0, 10, 8), (0, 0, 5000, 8)])      # wider than the distance transform
    shapes_, offsets = np.array([[5, 7], [3, 4]], np.int32), np.array([0, 35], np.int64)
    pts = np.zeros((2, 4, 2))
    with pytest.raises(ValueError):
        ops.active_contour_ragged(None, None, shapes_, offsets, pts, [4, 4], [0], np.zeros(16), [0, 0], None, None,
                                  0.01, 0.01, 5)
    with pytest.raises(ValueError):
        ops.active_contour_ragged(None, None, shapes_, offsets[:1], pts, [4, 4], [0, 1], np.zeros(16), [0, 0], None,
                                  None, 0.01, 0.01, 5)
    with pytest.raises(ValueError):
        ops.active_contour_ragged(None, None, shapes_, offsets, pts[0], [4, 4], [0, 1], np.zeros(16), [0, 0], None,
                                  None, 0.01, 0.01, 5)
    # the potentials of one call: 2-d, one dtype, uint8 or float32, and a known implementation
    f, u = np.zeros((5, 7), np.float32), np.zeros((3, 4), np.uint8)
    with pytest.raises(TypeError):
        ops.potential_gradients_ragged([f, u])
    with pytest.raises(TypeError):
        ops.potential_gradients_ragged([f.astype(np.float64)])
    with pytest.raises(ValueError):
        ops.potential_gradients_ragged([f, f[0]])
    with pytest.raises(ValueError):
        ops.potential_gradients_ragged([f], implementation="tiled")
    with pytest.raises(ValueError):
        ops.potential_gradients_ragged([f], sigma=-1.0)
    with pytest.raises(ValueError):
        ops.potential_gradients_ragged([u], 1.0, implementation="resident")
    big = np.zeros((ops.GRAD_RESIDENT_MAX_PIXELS + 1, 1), np.float32)
    with pytest.raises(ValueError):
        ops.potential_gradients_ragged([f, big], implementation="resident")
    # ActiveContour checks every item of a list as it checks a single potential
    ac = ActiveContour()
    with pytest.raises(ValueError):
        ac.set_potential([f, np.zeros((1, 9), np.float32)])
    with pytest.raises(TypeError):
        ac.set_potential([f, np.zeros((4, 9), np.float64)])
    with pytest.raises(TypeError):
        ac.set_potential([f, u])


def test_spline_helper_returns_what_the_method_returned():
    from video.analysis.shapes import Polygon, smooth_centerline
    fx = np.load(os.path.join(ROOT, "tests", "golden", "polygon_v1.npz"), allow_pickle=False)
    gentle = dict(alpha=10.0, beta=100.0, gamma=0.01, max_iterations=40)
    for name, kw in G.SMOOTH_CASES:
        # the fixture's centre line: the reference's own smoothed result (test_polygon_host.py's bound)
        got = np.asarray(smooth_centerline(fx["smooth/%s/points" % name], **kw))
        ref = fx["smooth/%s" % name]
        assert got.shape == ref.shape, name
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-9)
        # a centre line of the restatement: helper and method are one code
        points = G.optimized(G.FILL_POLYS[name], spacing=kw["spacing"], **gentle)
        via_method = np.asarray(Polygon(G.FILL_POLYS[name]).get_centerline_smoothed(points=points, **kw))
        via_helper = np.asarray(smooth_centerline(points, **kw))
        assert via_helper.shape == via_method.shape and len(via_helper) > 2, name
        assert np.array_equal(via_helper.view(np.uint64), via_method.view(np.uint64)), name
    # too short to skip both ends: the spline is not fitted and the (empty) middle comes back, as before
    short = np.array([[0.0, 0.0], [30.0, 0.0]])
    assert len(smooth_centerline(short, spacing=10, skip_length=90)) == 0
