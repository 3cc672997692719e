"""GPU: ActiveContour (va_snake.hip) bit-exact against the NumPy restatement of
tests/golden/make_golden_active_contour.py, and within 1e-8 px of the reference-run fixture.  Reads the npz and
the generator's restatement only."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_active_contour", os.path.join(ROOT, "tests", "golden", "make_golden_active_contour.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()


@pytest.fixture(scope="module")
def fx():
    from video import _hip
    _hip.lib()
    return np.load(os.path.join(ROOT, "tests", "golden", "active_contour_v1.npz"), allow_pickle=False)


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _model(name, params, closed, max_it):
    from video.analysis.active_contour import ActiveContour
    ac = ActiveContour(closed_loop=closed, **G.PARAMS[params])
    ac.max_iterations = max_it
    ac.residual_tolerance = G.TOLERANCE.get(name, 1)
    return ac


def _restated(ac, curve, anchor_x, anchor_y, frame=None):
    """the restatement run on the host preparation of the package and the gradients the GPU computed"""
    from video.analysis import curves
    pts = curves.make_curve_equidistant(curve)
    if len(pts) <= 2:
        return pts, None, None
    ds = curves.curve_length(pts) / (len(pts) - 1)
    flags, vals = ac._anchors(curve, pts, anchor_x, anchor_y)
    gx, gy = ac.fx, ac.fy
    if frame is not None:
        gx, gy = gx[frame], gy[frame]
    p, it, tv, _ = G.snake(gx, gy, pts, ac.get_evolution_matrix(len(pts), ds), ac.gamma,
                           ac.residual_tolerance * ac.gamma, ac.max_iterations, flags, vals)
    return p, it, tv


def test_sobel_planes_bit_identical(fx):
    from video import ops
    for dt, tag in ((np.uint8, "u8"), (np.float32, "f32")):
        for h, w in G.SOBEL_SIZES:
            x = G.sobel_input(h, w, dt, salt=h * 31 + w)
            gx, gy = ops.sobel5_f64(x)
            key = "sobel/%s_%dx%d" % (tag, h, w)
            assert _bits_equal(gx, fx[key + "/fx"]), key
            assert _bits_equal(gy, fx[key + "/fy"]), key
        # a stack, and one plane at a time
        x = np.stack([G.sobel_input(37, 53, dt, salt=s) for s in (1, 2, 3)])
        gx, gy = ops.sobel5_f64(x)
        for k in range(3):
            want = G.sobel5(x[k])
            assert _bits_equal(gx[k], want[0]) and _bits_equal(gy[k], want[1])
        assert ops.sobel5_f64(x, dx=False)[0] is None and _bits_equal(ops.sobel5_f64(x, dx=False)[1], gy)
        assert ops.sobel5_f64(x, dy=False)[1] is None and _bits_equal(ops.sobel5_f64(x, dy=False)[0], gx)


def test_sobel_random_shapes_bit_identical():
    from video import ops
    rng = np.random.default_rng(7)
    for h, w in ((1, 2), (2, 1), (3, 130), (17, 129), (33, 256), (70, 3)):
        for dt in (np.uint8, np.float32):
            x = (rng.integers(0, 256, (2, h, w)).astype(dt) if dt == np.uint8
                 else rng.normal(0, 30, (2, h, w)).astype(np.float32))
            gx, gy = ops.sobel5_f64(x)
            want = G.sobel5(x)
            assert _bits_equal(gx, want[0]) and _bits_equal(gy, want[1]), (h, w, dt)


def test_set_potential_gradients_bit_identical(fx):
    from video.analysis.active_contour import ActiveContour
    for dt, tag in ((np.uint8, "u8"), (np.float32, "f32")):
        p = G.sobel_input(48, 64, dt, salt=5)
        for s in G.BLUR_SIGMAS:
            ac = ActiveContour(blur_radius=s)
            ac.set_potential(p)
            key = "grad/%s_48x64_s%g" % (tag, s)
            assert G.sha(ac.fx) == fx[key + "/fx_sha"] and G.sha(ac.fy) == fx[key + "/fy_sha"], key
            assert _bits_equal(ac.fx.reshape(-1)[::7], fx[key + "/fx_sample"])
        # no blur: the Sobel planes of the potential itself
        ac = ActiveContour(blur_radius=0)
        ac.set_potential(p)
        want = G.sobel5(p)
        assert _bits_equal(ac.fx, want[0]) and _bits_equal(ac.fy, want[1])
    h, w, s = G.BIG
    ac = ActiveContour(blur_radius=s)
    ac.set_potential(G.big_input())
    for k, v in (("fx", ac.fx), ("fy", ac.fy)):
        assert v.shape == (h, w)
        assert _bits_equal(v.reshape(-1)[::G.SAMPLE_STRIDE], fx["grad/big/" + k + "_sample"])
        assert G.sha(v) == fx["grad/big/" + k + "_sha"]


def test_snakes_bit_identical_to_restatement_and_near_reference(fx):
    for name, pot, params, closed, N, max_it, ax, ay, kind in G.SNAKE_CASES:
        key = "snake/" + name
        ac = _model(name, params, closed, max_it)
        ac.set_potential(G.potential(pot))
        curve = fx[key + "/curve"]
        anchor_x, anchor_y = G.case_anchor(ax, N), G.case_anchor(ay, N)
        ac.info = {"iteration_count": -7}
        got = ac.find_contour(curve, anchor_x=anchor_x, anchor_y=anchor_y)
        p, it, tv = _restated(ac, curve, anchor_x, anchor_y)
        assert _bits_equal(got, p), name
        assert np.abs(got - fx[key + "/points"]).max() <= 1e-8, name
        if N <= 2:
            assert ac.info == {"iteration_count": -7}
            continue
        assert ac.info["iteration_count"] == it == fx[key + "/iterations"], name
        assert _bits_equal(ac.info["total_variation"], tv), name
        assert abs(ac.info["total_variation"] - fx[key + "/total_variation"]) <= 1e-8 * tv


def test_global_memory_path_and_lds_path_agree():
    """128 points are the last that keep the matrix in LDS; 129, 600 and 1024 points read it from global memory.
    All of them give what the restatement gives; 1025 points are refused"""
    ac = _model("x", "ref", True, 50)
    ac.set_potential(G.potential("f32"))
    for N in (128, 129, 600, 1024):
        curve = G.ellipse_curve(N, True)
        got = ac.find_contour(curve)
        p, it, tv = _restated(ac, curve, None, None)
        assert _bits_equal(got, p) and ac.info["iteration_count"] == it, N
    with pytest.raises(ValueError):
        ac.find_contour(G.ellipse_curve(1025, True))


def test_batch_equals_per_call():
    from video.analysis.active_contour import ActiveContour
    ac = ActiveContour(blur_radius=2.5, closed_loop=False)
    ac.max_iterations = 300
    ac.residual_tolerance = 2000
    stack = np.stack([G.potential("f32"), G.potential("f32_soft"), G.potential("f32")[::-1].copy()])
    ac.set_potential(stack)
    curves_, frames, axs, ays = [], [], [], []
    for k, (N, scale, frame) in enumerate(((64, 1.05, 0), (600, 1.1, 1), (5, 1.0, 2), (2, 1.0, 0), (64, 1.05, 0),
                                           (200, 0.95, 1), (64, 1.05, 2), (1, 1.0, 1))):
        curves_.append(G.ellipse_curve(N, False, scale=scale))
        frames.append(frame)
        axs.append([0] if k % 3 == 0 else None)
        ays.append(np.arange(N) == N - 1 if k % 2 == 0 and N > 2 else None)
    batch = ac.find_contours(curves_, frames, axs, ays)
    its, tvs = ac.info["iteration_count"].copy(), ac.info["total_variation"].copy()
    assert len(set(its.tolist())) > 2
    for k in range(len(curves_)):
        one = ac.find_contour(curves_[k], axs[k], ays[k], frame=frames[k])
        assert _bits_equal(batch[k], one), k
        if len(one) > 2:
            assert its[k] == ac.info["iteration_count"] and _bits_equal(tvs[k], ac.info["total_variation"])
            p, it, tv = _restated(ac, curves_[k], axs[k], ays[k], frame=frames[k])
            assert _bits_equal(one, p) and it == its[k], k
        else:
            assert its[k] == 0 and tvs[k] == 0.0
    with pytest.raises(IndexError):
        ac.find_contours(curves_[:1], [3])


def test_two_calls_back_to_back_on_a_created_stream():
    """contours of different lengths on a non-blocking stream, through the wrappers and as two launches
    enqueued back to back on one set of gradients"""
    from video import _hip, ops
    from video._hip import check
    from video.analysis import curves
    from video.analysis.active_contour import ActiveContour
    L = _hip.lib()
    stream = C.c_void_p()
    check(L.va_stream_create(C.byref(stream)))
    ac = ActiveContour(blur_radius=10)
    try:
        p = G.potential("u8")
        gx, gy, shape = ops.potential_gradients(p, 10.0, stream)
        ac.set_potential(p)
        want_gx, want_gy = ac.fx, ac.fy
        assert _bits_equal(gx.download(shape, np.float64), want_gx[None])
        jobs = []
        for N in (600, 64, 200, 5):
            pts = curves.make_curve_equidistant(G.ellipse_curve(N, True))
            ds = curves.curve_length(pts) / (N - 1)
            jobs.append((pts, ac.get_evolution_matrix(N, ds)))
        for pts, P in jobs:
            out, it, tv = ops.active_contour(gx, gy, shape, pts[None], [len(pts)], [0], P.T.reshape(-1), [0], None,
                                             None, ac.gamma, ac.gamma, 50, stream)
            q, it_w, tv_w, _ = G.snake(want_gx, want_gy, pts, P, ac.gamma, ac.gamma, 50)
            assert _bits_equal(out[0], q) and it[0] == it_w and _bits_equal(tv[0], tv_w)
        # raw: both launches enqueued before the stream is synchronised
        bufs, outs = [], []
        for pts, P in jobs[:2]:
            N = len(pts)
            arrs = [np.ascontiguousarray(pts), np.array([N], np.int32), np.array([0], np.int32),
                    np.ascontiguousarray(P.T).reshape(-1), np.array([0], np.int64)]
            b = [_hip.DeviceBuffer.from_array(a, stream) for a in arrs]
            it_b, tv_b = _hip.DeviceBuffer(4), _hip.DeviceBuffer(8)
            bufs.append((b, it_b, tv_b, N, arrs[3].size))
        for b, it_b, tv_b, N, msize in bufs:
            check(L.va_active_contour(gx.ptr, gy.ptr, 1, shape[1], shape[2], 1, N, b[1].ptr, b[2].ptr, b[3].ptr,
                                      b[4].ptr, msize, None, None, ac.gamma, ac.gamma, 50, b[0].ptr, it_b.ptr,
                                      tv_b.ptr, stream))
        check(L.va_stream_sync(stream))
        for (b, it_b, tv_b, N, _), (pts, P) in zip(bufs, jobs[:2]):
            q, it_w, _, _ = G.snake(want_gx, want_gy, pts, P, ac.gamma, ac.gamma, 50)
            assert _bits_equal(b[0].download((N, 2), np.float64), q)
            assert it_b.download((1,), np.int32)[0] == it_w
        gx.free()
        gy.free()
    finally:
        check(L.va_stream_destroy(stream))


def test_error_codes():
    from video import _hip, ops
    from video.analysis.active_contour import ActiveContour
    L = _hip.lib()
    buf = _hip.DeviceBuffer(1 << 16)
    p = buf.ptr
    assert L.va_sobel5_f64(p, _hip.VA_F64, p, p, 1, 8, 8, None) == -22
    assert L.va_sobel5_f64(None, _hip.VA_U8, p, p, 1, 8, 8, None) == -22
    assert L.va_sobel5_f64(p, _hip.VA_U8, None, None, 1, 8, 8, None) == -22
    assert L.va_sobel5_f64(p, _hip.VA_U8, p, p, 1, 0, 8, None) == -22
    assert L.va_sobel5_f64(p, _hip.VA_U8, p, p, 0, 8, 8, None) == 0

    def snake_call(n=1, h=8, w=8, m=1, max_points=8, max_it=5, mats_count=64, flags=None, vals=None, ptr=p):
        return L.va_active_contour(ptr, ptr, n, h, w, m, max_points, ptr, ptr, ptr, ptr, mats_count, flags, vals,
                                   0.001, 0.001, max_it, ptr, ptr, ptr, None)
    assert snake_call(h=1) == -22
    assert snake_call(w=1) == -22
    assert snake_call(n=0) == -22
    assert snake_call(max_points=ops.SNAKE_MAX_POINTS + 1) == -22
    assert snake_call(max_it=0) == -22
    assert snake_call(mats_count=-1) == -22
    assert snake_call(flags=p, vals=None) == -22
    assert snake_call(ptr=None) == -22
    assert snake_call(m=0, ptr=None) == 0
    # entries out of range are refused on the device (iterations -1), nothing is read or written for them
    ac = ActiveContour(blur_radius=1)
    ac.set_potential(G.potential("f32"))
    gx, gy, shape = ac._grad
    pts = np.zeros((4, 8, 2))
    P = np.eye(8).reshape(-1)
    for case, (npts, frames, offs) in enumerate((([8], [1], [0]), ([8], [-1], [0]), ([8], [0], [1]),
                                                  ([9], [0], [0]))):
        out, it, tv = ops.active_contour(gx, gy, shape, pts[:1], npts, frames, P, offs, None, None, 0.001, 0.001, 5)
        assert it[0] == -1 and np.array_equal(out, pts[:1]), case
    with pytest.raises(TypeError):
        ops.sobel5_f64(np.zeros((8, 8), np.float64))
    with pytest.raises(ValueError):
        ac.find_contour(np.array([[0.0, 0.0], [np.nan, 1.0], [3.0, 3.0]]))
