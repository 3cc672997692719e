"""GPU: the batched centre lines -- ragged blur + Sobel (va_potential_gradients_ragged), snakes on ragged planes
(va_active_contour_ragged) and video.analysis.shapes.get_centerlines_optimized / _smoothed -- bit for bit against
the NumPy restatements of tests/golden/make_golden_polygon.py and make_golden_active_contour.py, and against the
per-polygon methods.  Comparisons are on the bit patterns, so signed zeros count."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator("make_golden_polygon")
ACG = _generator("make_golden_active_contour")

# the odd pixel counts come first, so that later offsets are odd
GRAD_SHAPES = ((3, 3), (2, 13), (10, 2), (1, 7), (5, 5), (6, 9), (27, 82), (37, 53), (56, 62))
GRAD_SIGMAS = (0.0, 1.0, 2.5)      # radius 4 and 10: wider than several items

CHAIN_PARAMS = (dict(alpha=10., beta=100., gamma=0.01, spacing=5, max_iterations=60),
                dict(alpha=100., beta=1e3, gamma=0.01, spacing=6, max_iterations=50),
                dict())
CHAIN_ENDPOINTS = {"l_shape": [[5, 3], [29, 33]]}


@pytest.fixture(scope="module")
def gpu():
    from video import _hip
    return _hip.lib()


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _planes(grads):
    """the per-item (fx, fy) arrays of what potential_gradients_ragged returns; frees the device planes"""
    fx, fy, shapes, offsets = grads
    total = int((shapes[:, 0].astype(np.int64) * shapes[:, 1]).sum())
    out = []
    try:
        flats = [b.download((total,), np.float64) for b in (fx, fy)]
    finally:
        fx.free()
        fy.free()
    for (h, w), o in zip(shapes.tolist(), offsets.tolist()):
        out.append(tuple(f[o:o + h * w].reshape(h, w) for f in flats))
    return out


def _grad_items(dtype):
    return [ACG.sobel_input(h, w, dtype, salt=7 * k + 1) for k, (h, w) in enumerate(GRAD_SHAPES)]


# ------------------------------------------------------------------------------------- ragged gradients
@pytest.fixture(scope="module")
def grad_reference():
    """ACG.gradients of every float32 item and sigma, computed once"""
    return {s: [ACG.gradients(p, s) for p in _grad_items(np.float32)] for s in GRAD_SIGMAS}


@pytest.mark.parametrize("sigma", GRAD_SIGMAS)
def test_ragged_gradients_equal_restatement(gpu, grad_reference, sigma):
    from video import ops
    items = _grad_items(np.float32)
    fx, fy, shapes, offsets = grads = ops.potential_gradients_ragged(items, sigma)
    assert shapes.tolist() == [list(s) for s in GRAD_SHAPES]
    assert offsets.tolist() == np.concatenate([[0], np.cumsum([h * w for h, w in GRAD_SHAPES])[:-1]]).tolist()
    assert sum(o % 2 for o in offsets.tolist()) >= 3          # odd offsets are covered
    got = _planes(grads)
    for k, (p, g, want) in enumerate(zip(items, got, grad_reference[sigma])):
        assert _bits_equal(g[0], want[0]) and _bits_equal(g[1], want[1]), (sigma, k, p.shape)
    # forced onto the kernel: the same bits
    forced = _planes(ops.potential_gradients_ragged(items, sigma, implementation="resident"))
    for k, (g, f) in enumerate(zip(got, forced)):
        assert _bits_equal(g[0], f[0]) and _bits_equal(g[1], f[1]), (sigma, k)
    # each item alone, and the stack path of each item
    for k, (p, g) in enumerate(zip(items, got)):
        alone = _planes(ops.potential_gradients_ragged([p], sigma))[0]
        assert _bits_equal(alone[0], g[0]) and _bits_equal(alone[1], g[1]), (sigma, k)
        sx, sy, shape = ops.potential_gradients(p, sigma)
        try:
            assert _bits_equal(sx.download(shape, np.float64)[0], g[0]), (sigma, k)
            assert _bits_equal(sy.download(shape, np.float64)[0], g[1]), (sigma, k)
        finally:
            sx.free()
            sy.free()


def test_ragged_gradients_uint8(gpu):
    from video import ops
    items = _grad_items(np.uint8)
    got = _planes(ops.potential_gradients_ragged(items, 0.0, implementation="resident"))
    for k, (p, g) in enumerate(zip(items, got)):
        want = ACG.gradients(p, 0)
        assert _bits_equal(g[0], want[0]) and _bits_equal(g[1], want[1]), k
    # with a blur the 8-bit items take the fixed-point va_gaussian_u8, one by one
    got = _planes(ops.potential_gradients_ragged(items, 1.0))
    for k, (p, g) in enumerate(zip(items, got)):
        want = ACG.gradients(p, 1.0)
        assert _bits_equal(g[0], want[0]) and _bits_equal(g[1], want[1]), k
    with pytest.raises(ValueError):
        ops.potential_gradients_ragged(items, 1.0, implementation="resident")
    with pytest.raises(TypeError):
        ops.potential_gradients_ragged([items[0], items[1].astype(np.float32)])


@pytest.mark.parametrize("sigma", (0.0, 1.0))
def test_ragged_gradients_above_the_resident_limit(gpu, sigma):
    from video import ops
    limit = ops.GRAD_RESIDENT_MAX_PIXELS
    small = _grad_items(np.float32)[:3]
    at = ACG.sobel_input(limit, 1, np.float32, salt=3)           # the largest item the kernel takes
    above = ACG.sobel_input(limit + 1, 1, np.float32, salt=4)    # one pixel more: a single tall strip
    items = small + [at, above, small[0]]
    got = _planes(ops.potential_gradients_ragged(items, sigma))
    for k, (p, g) in enumerate(zip(items, got)):
        want = ACG.gradients(p, sigma)
        assert _bits_equal(g[0], want[0]) and _bits_equal(g[1], want[1]), (sigma, k, p.shape)
    _planes(ops.potential_gradients_ragged(small + [at], sigma, implementation="resident"))
    with pytest.raises(ValueError):
        ops.potential_gradients_ragged(items, sigma, implementation="resident")


# --------------------------------------------------------------------------------------- ragged snakes
def _snake_potentials():
    """three crops of different shapes: two the resident kernel takes, one above its limit"""
    return [ACG.potential("f32")[:60, :80].copy(), ACG.potential("f32_soft")[20:65, 30:130].copy(),
            ACG.potential("f32")[10:110, 15:146].copy()]


def _snake_jobs(closed):
    """(curve, item, anchor_x, anchor_y) spread over the three items"""
    half = lambda c: c * 0.5                                   # noqa: E731
    jobs = [(half(ACG.ellipse_curve(40, closed)), 0, None, None),
            (ACG.ellipse_curve(64, closed) - [30.0, 20.0], 1, None, None),
            (ACG.ellipse_curve(70, closed) - [15.0, 10.0], 2, None, None),
            (half(ACG.ellipse_curve(5, closed)), 0, None, None),
            (ACG.ellipse_curve(150, closed, scale=1.6) - [15.0, 10.0], 2, None, None),      # partly outside: clipped
            (half(ACG.ellipse_curve(2, closed)), 1, None, None)]
    if not closed:
        jobs += [(half(ACG.ellipse_curve(48, False)), 0, [0, 47], [0, 47]),
                 (ACG.ellipse_curve(64, False) - [30.0, 20.0], 1, [0, 20, 63], None),
                 (ACG.clustered_curve(40) - [15.0, 10.0], 2, [0, 1, 2, 3, 2, 39], [5, 4, 0, 1])]
    return jobs


@pytest.mark.parametrize("closed", (False, True))
def test_ragged_snakes_equal_single_items_and_restatement(gpu, closed):
    from video.analysis import curves
    from video.analysis.active_contour import ActiveContour
    pots, jobs = _snake_potentials(), _snake_jobs(closed)
    ac = ActiveContour(closed_loop=closed, **ACG.PARAMS["ref"])
    ac.set_potential(pots)
    assert isinstance(ac.fx, list) and [g.shape for g in ac.fx] == [p.shape for p in pots]
    got = ac.find_contours([j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs], [j[3] for j in jobs])
    its, tvs = ac.info["iteration_count"].copy(), ac.info["total_variation"].copy()
    singles = []
    for p in pots:
        one = ActiveContour(closed_loop=closed, **ACG.PARAMS["ref"])
        one.set_potential(p)
        singles.append(one)
    for k, (curve, item, ax, ay) in enumerate(jobs):
        one = singles[item]
        assert _bits_equal(ac.fx[item], one.fx) and _bits_equal(ac.fy[item], one.fy), (k, item)
        one.info = {}
        want = one.find_contour(curve, anchor_x=ax, anchor_y=ay)
        assert _bits_equal(got[k], want), (closed, k)
        # the restatement on the downloaded planes of the batch
        pts = curves.make_curve_equidistant(curve)
        if len(pts) <= 2:
            assert _bits_equal(got[k], pts) and its[k] == 0 and tvs[k] == 0.0
            continue
        assert its[k] == one.info["iteration_count"] and _bits_equal(tvs[k], one.info["total_variation"]), (closed, k)
        ds = curves.curve_length(pts) / (len(pts) - 1)
        flags, vals = ac._anchors(curve, pts, ax, ay)
        p, it, tv, _ = ACG.snake(ac.fx[item], ac.fy[item], pts, ac.get_evolution_matrix(len(pts), ds), ac.gamma,
                                 ac.residual_tolerance * ac.gamma, ac.max_iterations, flags, vals)
        assert _bits_equal(got[k], p) and its[k] == it and _bits_equal(tvs[k], tv), (closed, k)
    with pytest.raises(IndexError):
        ac.find_contours([jobs[0][0]], [3])


# ------------------------------------------------------------------------------------- the whole chain
@pytest.fixture(scope="module")
def chain_reference():
    """G.optimized of the fifteen polygons for each parameter set, computed once"""
    return [[G.optimized(c, endpoints=CHAIN_ENDPOINTS.get(name), **params) for name, c in G.FILL_POLYS.items()]
            for params in CHAIN_PARAMS]


@pytest.mark.parametrize("case", range(len(CHAIN_PARAMS)))
def test_centerlines_optimized_equal_restatement_and_single_polygons(gpu, chain_reference, case):
    from video.analysis.shapes import Polygon, get_centerlines_optimized
    params = CHAIN_PARAMS[case]
    names = list(G.FILL_POLYS)
    assert len(names) == 15
    polygons = [Polygon(G.FILL_POLYS[n]) for n in names]
    endpoints = [CHAIN_ENDPOINTS.get(n) for n in names]
    got = get_centerlines_optimized(polygons, endpoints=endpoints, **params)
    assert len(got) == 15
    for name, poly, ep, g, want in zip(names, polygons, endpoints, got, chain_reference[case]):
        assert _bits_equal(g, want), (case, name)
        assert _bits_equal(g, poly.get_centerline_optimized(endpoints=ep, **params)), (case, name)


def test_centerlines_smoothed_equal_single_polygons(gpu):
    from video.analysis.shapes import Polygon, get_centerlines, get_centerlines_smoothed
    polys = {name: Polygon(G.FILL_POLYS[name]) for name, _ in G.SMOOTH_CASES}
    for name, kw in G.SMOOTH_CASES:
        want = polys[name].get_centerline_smoothed(**kw)
        others = [polys[n] for n, _ in G.SMOOTH_CASES if n != name]
        got = get_centerlines_smoothed([polys[name]] + others, **kw)
        assert len(got) == 3 and _bits_equal(got[0], want), name
        assert _bits_equal(get_centerlines([polys[name]], **kw)[0], polys[name].get_centerline(**kw)), name
        assert _bits_equal(get_centerlines([polys[name]], method="smoothed", **kw)[0], want), name
    ps = list(polys.values())
    kw = dict(spacing=5, max_iterations=40)
    for g, p in zip(get_centerlines(ps, method="optimized", **kw), ps):
        assert _bits_equal(g, p.get_centerline(method="optimized", **kw))
    for g, p in zip(get_centerlines(ps, method="estimate"), ps):
        assert np.array_equal(g, p.get_centerline(method="estimate"))
    with pytest.raises(ValueError):
        get_centerlines(ps, method="nope")


# ------------------------------------------------------------------------------------ errors and limits
def test_item_out_of_range_leaves_the_contour(gpu):
    from video import ops
    from video.analysis import curves
    from video.analysis.active_contour import ActiveContour
    pots = _snake_potentials()[:2]
    fx, fy, shapes, offsets = ops.potential_gradients_ragged(pots, 1.0)
    try:
        ac = ActiveContour(**ACG.PARAMS["ref"])
        pts = curves.make_curve_equidistant(ACG.ellipse_curve(20, False) * 0.5)
        N = len(pts)
        mat = np.ascontiguousarray(ac.get_evolution_matrix(N, curves.curve_length(pts) / (N - 1)).T).reshape(-1)
        table = np.stack([pts, pts, pts, pts])
        for items, bad in (([0, 2, 1, -1], [1, 3]), ([5, 0, 0, 1], [0])):
            out, its, tvs = ops.active_contour_ragged(fx, fy, shapes, offsets, table, [N] * 4, items, mat, [0] * 4,
                                                      None, None, ac.gamma, ac.gamma, 20)
            for k in range(4):
                if k in bad:
                    assert its[k] == -1 and _bits_equal(out[k], pts), (items, k)
                else:
                    assert its[k] >= 1 and not _bits_equal(out[k], pts), (items, k)
        # an item too small for a snake, and a plane that does not fit in the buffer
        tiny = np.array([[1, 9], [60, 80]], np.int32)
        out, its, _ = ops.active_contour_ragged(fx, fy, tiny, np.array([0, 9], np.int64), table[:2], [N] * 2, [0, 1],
                                                mat, [0] * 2, None, None, ac.gamma, ac.gamma, 20)
        assert its[0] == -1 and its[1] >= 1 and _bits_equal(out[0], pts)
        out, its, _ = ops.active_contour_ragged(fx, fy, tiny, np.array([0, 10], np.int64), table[:2], [N] * 2, [1, 1],
                                                mat, [0] * 2, None, None, ac.gamma, ac.gamma, 20)
        assert its.tolist() == [-1, -1] and _bits_equal(out[1], pts)
        with pytest.raises(ValueError):
            ops.active_contour_ragged(fx, fy, shapes, offsets, table, [N] * 3, [0] * 4, mat, [0] * 4, None, None,
                                      ac.gamma, ac.gamma, 20)
    finally:
        fx.free()
        fy.free()


def test_entry_point_argument_checks(gpu):
    from video import _hip, ops
    L = gpu
    p = C.c_void_p(16)                   # never dereferenced: the checks come first
    grad = lambda dtype, total, m, max_pixels, sigma, src=p: L.va_potential_gradients_ragged(   # noqa: E731
        src, dtype, p, p, total, m, max_pixels, sigma, p, p, p, None)
    assert grad(_hip.VA_U8, 8, 1, 8, 1.0) == -22             # the 8-bit blur is not this kernel's
    assert grad(_hip.VA_F64, 8, 1, 8, 0.0) == -22
    assert grad(_hip.VA_F32, 8, 1, 8, -1.0) == -22
    assert grad(_hip.VA_F32, 8, -1, 8, 0.0) == -22
    assert grad(_hip.VA_F32, -8, 1, 8, 0.0) == -22
    assert grad(_hip.VA_F32, 8, 1, ops.GRAD_RESIDENT_MAX_PIXELS + 1, 0.0) == -22
    assert grad(_hip.VA_F32, 8, 1, 8, 0.0, src=None) == -22
    assert grad(_hip.VA_F32, 8, 0, 8, 1.0) == 0              # no items: nothing is launched
    assert grad(_hip.VA_U8, 0, 0, 0, 0.0, src=None) == 0
    snake = lambda total, n_items, m, max_points, max_it, pts=p: L.va_active_contour_ragged(    # noqa: E731
        p, p, p, p, total, n_items, m, max_points, p, p, p, p, 16, None, None, 0.01, 0.01, max_it, pts, p, p, None)
    assert snake(64, 1, 1, 2000, 5) == -22
    assert snake(64, 1, 1, 0, 5) == -22
    assert snake(64, 1, 1, 8, 0) == -22
    assert snake(-1, 1, 1, 8, 5) == -22
    assert snake(64, -1, 1, 8, 5) == -22
    assert snake(64, 1, 1, 8, 5, pts=None) == -22
    assert snake(64, 1, 0, 8, 5) == 0


def test_empty_calls(gpu):
    from video import ops
    from video.analysis.shapes import get_centerlines, get_centerlines_optimized, get_centerlines_smoothed
    for grads in (ops.potential_gradients_ragged([]), ops.centerline_gradients([], [])):
        fx, fy, shapes, offsets = grads
        assert shapes.shape == (0, 2) and offsets.shape == (0,)
        out, its, tvs = ops.active_contour_ragged(fx, fy, shapes, offsets, np.zeros((0, 4, 2)), [], [], np.zeros(0), [],
                                                  None, None, 0.01, 0.01, 5)
        assert out.shape == (0, 4, 2) and its.shape == (0,) and tvs.shape == (0,)
        assert _planes(grads) == []
    assert get_centerlines_optimized([]) == [] and get_centerlines_smoothed([]) == [] and get_centerlines([]) == []
    # empty items among others are left alone
    items = [np.zeros((0, 5), np.float32), ACG.sobel_input(5, 5, np.float32), np.zeros((4, 0), np.float32)]
    got = _planes(ops.potential_gradients_ragged(items, 1.0, implementation="resident"))
    want = ACG.gradients(items[1], 1.0)
    assert got[0][0].shape == (0, 5) and got[2][0].shape == (4, 0)
    assert _bits_equal(got[1][0], want[0]) and _bits_equal(got[1][1], want[1])


def test_back_to_back_calls_on_a_created_stream(gpu):
    from video import ops
    L = gpu
    names = ("worm", "mouse", "l_shape", "tiny")
    sets = []
    for margin in (1, 3):
        boxes = [G.bounding_rect(G.FILL_POLYS[n], margin) for n in names]
        sets.append(([np.asarray(G.FILL_POLYS[n]).astype(np.int64) for n in names], boxes))
    want = [_planes(ops.centerline_gradients(c, b)) for c, b in sets]
    s = C.c_void_p()
    assert L.va_stream_create(C.byref(s)) == 0
    try:
        held = [ops.centerline_gradients(c, b, stream=s.value) for c, b in sets]     # both alive at once
        got = [_planes(g) for g in held]
    finally:
        L.va_stream_destroy(s.value)
    for a, b in zip(got, want):
        for (gx, gy), (wx, wy) in zip(a, b):
            assert _bits_equal(gx, wx) and _bits_equal(gy, wy)
    # and the chain's planes are those of the restatement
    for (gx, gy), n in zip(want[0], names):
        mask, _ = G.get_mask(G.FILL_POLYS[n], 1)
        wx, wy = ACG.gradients(G.distance_transform(mask), 1)
        assert _bits_equal(gx, wx) and _bits_equal(gy, wy), n
