"""CPU: the active-contour fixture (tests/golden/active_contour_v1.npz) is complete and the NumPy restatement
of tests/golden/make_golden_active_contour.py reproduces it; the host helpers (video.analysis.curves,
image.subpixel(s), ActiveContour.get_evolution_matrix) equal what the reference's own code computed;
ActiveContour refuses what it cannot run and fails loudly without a GPU."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gen():
    spec = importlib.util.spec_from_file_location(
        "make_golden_active_contour", os.path.join(ROOT, "tests", "golden", "make_golden_active_contour.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _gen()


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "active_contour_v1.npz"), allow_pickle=False)


def _prepare(ac, curve, anchor_x, anchor_y):
    """the package's host preparation of one contour: equidistant points, matrix, anchor arrays"""
    from video.analysis import curves
    pts = curves.make_curve_equidistant(curve)
    ds = curves.curve_length(pts) / (len(pts) - 1)
    flags, vals = ac._anchors(curve, pts, anchor_x, anchor_y)
    return pts, ac.get_evolution_matrix(len(pts), ds), flags, vals


def test_fixture_is_complete(fixture):
    keys = set(fixture.files)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "active_contour_v1.npz")) <= 350 * 1024
    for tag in ("u8", "f32"):
        for h, w in G.SOBEL_SIZES:
            assert fixture["sobel/%s_%dx%d/fx" % (tag, h, w)].shape == (h, w)
            assert fixture["sobel/%s_%dx%d/fy" % (tag, h, w)].dtype == np.float64
        for s in G.BLUR_SIGMAS:
            for k in ("fx", "fy"):
                assert "grad/%s_48x64_s%g/%s_sha" % (tag, s, k) in keys
    for k in ("fx", "fy"):
        assert "grad/big/%s_sha" % k in keys and "grad/big/%s_sample" % k in keys
    for N, ds, params, closed in G.MATRIX_CASES:
        assert fixture["matrix/%d_%g_%s_%d" % (N, ds, params, closed)].shape == (N, N)
    kept = list(fixture["snake_kept"])
    assert kept == [c[0] for c in G.SNAKE_CASES], "a snake case was dropped for its margin"
    seen = set()
    for name, pot, params, closed, N, max_it, ax, ay, kind in G.SNAKE_CASES:
        key = "snake/" + name
        assert fixture[key + "/points"].shape == (N, 2)
        if N > 2:
            assert fixture[key + "/margin"] >= G.MIN_MARGIN
            it = int(fixture[key + "/iterations"])
            assert 1 <= it <= max_it
            seen.add("stopped early" if it < max_it else "ran out")
        seen.update([params, "closed" if closed else "open", "max%d" % max_it])
        seen.update(["N%d" % N] if N in (3, 4, 5, 64, 200, 600) or N <= 2 else [])
    assert {"ref", "centre", "open", "closed", "max1", "max50", "max1000", "stopped early", "ran out",
            "N3", "N4", "N5", "N64", "N200", "N600", "N2", "N1"} <= seen


def test_restated_sobel_reproduces_fixture(fixture):
    for dt, tag in ((np.uint8, "u8"), (np.float32, "f32")):
        for h, w in G.SOBEL_SIZES:
            fx, fy = G.sobel5(G.sobel_input(h, w, dt, salt=h * 31 + w))
            key = "sobel/%s_%dx%d" % (tag, h, w)
            assert np.array_equal(fx.view(np.uint64), fixture[key + "/fx"].view(np.uint64))
            assert np.array_equal(fy.view(np.uint64), fixture[key + "/fy"].view(np.uint64))
        p = G.sobel_input(48, 64, dt, salt=5)
        for s in G.BLUR_SIGMAS:
            fx, fy = G.gradients(p, s)
            key = "grad/%s_48x64_s%g" % (tag, s)
            assert G.sha(fx) == fixture[key + "/fx_sha"] and G.sha(fy) == fixture[key + "/fy_sha"]


def test_restated_sobel_is_a_derivative():
    """on a quadratic ramp away from the border both planes are exact multiples of the derivative"""
    y, x = np.mgrid[:20, :24].astype(np.float32)
    p = (0.5 * x * x + 3 * y).astype(np.float32)
    fx, fy = G.sobel5(p)
    # the 5-tap kernels: d/dx weight 8 * 16 (row [-1 -2 0 2 1] -> 8 x', column [1 4 6 4 1] sums to 16)
    assert np.array_equal(fx[2:-2, 2:-2], 128.0 * x[2:-2, 2:-2])
    assert np.array_equal(fy[2:-2, 2:-2], np.full((16, 20), 128.0 * 3))
    # a constant image has zero gradients of positive sign (the +0.0 delta)
    fx, fy = G.sobel5(np.full((5, 6), 7, np.uint8))
    assert not np.signbit(fx).any() and not np.signbit(fy).any() and not fx.any() and not fy.any()


def test_curves_and_subpixels_match_reference(fixture):
    from video.analysis import curves, image
    for name in G.HELPER_CURVES:
        c = fixture["curves/%s/in" % name]
        k = "curves/%s/" % name
        assert curves.curve_length(c) == fixture[k + "length"]
        assert np.array_equal(curves.curve_segment_lengths(c), fixture[k + "segments"])
        assert np.array_equal(curves.make_curve_equidistant(c), fixture[k + "equidistant"])
        assert np.array_equal(curves.make_curve_equidistant(c, count=11), fixture[k + "equidistant_count"])
        assert np.array_equal(np.asarray(curves.make_curve_equidistant(c, spacing=2.5)),
                              fixture[k + "equidistant_spacing"])
        assert np.array_equal(curves.translate_points(c, 1.5, -2.0), fixture[k + "translated"])
        assert curves.point_distance(c[0], c[1]) == fixture[k + "distance01"]
    assert curves.curve_length([[1.0, 2.0]]) == 0
    assert curves.translate_points([(1, 2)], 1, 1) == [(2, 3)]
    img, pts = fixture["image/img"], fixture["image/pts"]
    assert np.array_equal(image.subpixels(img, pts), fixture["image/subpixels"])
    assert np.array_equal(np.array([image.subpixel(img, p) for p in pts]), fixture["image/subpixel"])


def test_curve_length_is_the_float32_restatement():
    """arcLength's float32 terms differ from np.hypot in double: the restatement must keep them"""
    from video.analysis import curves
    c = np.array([[0.1, 0.2], [1.3, 2.7], [4.4, 3.3], [7.7, 9.1]])
    seg = np.sqrt(np.sum(np.diff(c.astype(np.float32), axis=0) ** 2, axis=1, dtype=np.float32))
    assert curves.curve_length(c) == float(np.cumsum(seg.astype(np.float64))[-1])
    assert curves.curve_length(c) != float(np.sum(np.hypot(*np.diff(c, axis=0).T)))


def test_evolution_matrix_matches_reference(fixture):
    from video.analysis.active_contour import ActiveContour
    for N, ds, params, closed in G.MATRIX_CASES:
        pr = dict(G.PARAMS[params])
        pr.pop("blur_radius")
        P = ActiveContour(blur_radius=0, closed_loop=closed, **pr).get_evolution_matrix(N, ds)
        want = fixture["matrix/%d_%g_%s_%d" % (N, ds, params, closed)]
        assert np.all(np.abs(P - want) <= 1e-15 * np.abs(want).max()), (N, ds, params, closed)


def test_restated_snake_matches_reference_run(fixture):
    from video.analysis.active_contour import ActiveContour
    grads = {}
    for name, pot, params, closed, N, max_it, ax, ay, kind in G.SNAKE_CASES:
        key = "snake/" + name
        curve = fixture[key + "/curve"]
        if N <= 2:
            from video.analysis import curves
            assert np.array_equal(curves.make_curve_equidistant(curve), fixture[key + "/points"])
            continue
        pr = G.PARAMS[params]
        fx, fy = grads.setdefault((pot, pr["blur_radius"]), G.gradients(G.potential(pot), pr["blur_radius"]))
        ac = ActiveContour(closed_loop=closed, **pr)
        pts, P, flags, vals = _prepare(ac, curve, G.case_anchor(ax, N), G.case_anchor(ay, N))
        tol = G.TOLERANCE.get(name, 1) * ac.gamma
        p, it, tv, margin = G.snake(fx, fy, pts, P, ac.gamma, tol, max_it, flags, vals)
        assert it == fixture[key + "/iterations"], name
        assert np.abs(p - fixture[key + "/points"]).max() <= 1e-8, name
        assert abs(tv - fixture[key + "/total_variation"]) <= 1e-8 * max(1.0, abs(tv)), name
        assert margin >= G.MIN_MARGIN


def test_anchor_duplicates_resolve_last_wins():
    from video.analysis import curves
    from video.analysis.active_contour import ActiveContour
    curve = G.clustered_curve(40)
    pts = curves.make_curve_equidistant(curve)
    anchors = [0, 1, 2, 3, 2, 39]
    flags, vals = ActiveContour._anchors(curve, pts, anchors, None)
    want_flags, want_vals = np.zeros(40, np.uint8), np.zeros(40)
    for a in anchors:                         # one by one: a later anchor on the same point overwrites
        i = int(np.argmin([np.hypot(*(p - curve[a])) for p in pts]))
        want_flags[i], want_vals[i] = 1, curve[a, 0]
    assert np.array_equal(flags, want_flags) and np.array_equal(vals[:, 0], want_vals)
    assert flags.sum() < len(set(anchors))    # the case does put two anchors on one point
    flags, vals = ActiveContour._anchors(curve, pts, None, np.arange(40) == 39)
    assert flags[39] == 2 and vals[39, 1] == curve[39, 1] and flags[:39].sum() == 0
    assert ActiveContour._anchors(curve, pts, None, None) == (None, None)


def test_reduction_order_is_fixed():
    e = np.array([1e16, 1.0, -1e16] + [0.0] * 300 + [1.0])
    # thread 0 adds e[0] + e[256]; thread 1 e[1] + e[257]; ... then halves
    acc = np.zeros(256)
    acc[:len(e) - 256] += e[256:]
    acc = e[:256] + acc
    while len(acc) > 1:
        acc = acc[:len(acc) // 2] + acc[len(acc) // 2:]
    assert G.fixed_sum(e) == acc[0]
    assert G.fixed_sum(np.array([])) == 0.0


def test_model_refuses_what_it_cannot_run():
    from video import _hip
    from video.analysis.active_contour import ActiveContour
    ac = ActiveContour()
    assert ac.fx is None and ac.fy is None and ac.info == {}
    assert (ActiveContour.max_iterations, ActiveContour.max_cache_count, ActiveContour.residual_tolerance) == \
        (50, 20, 1)
    with pytest.raises(RuntimeError, match="Potential must be set"):
        ac.find_contour([[1, 2], [3, 4], [5, 6]])
    with pytest.raises(RuntimeError):
        ac.find_contours([[[1, 2], [3, 4], [5, 6]]])
    for bad in (np.zeros((8, 8)), np.zeros((8, 8), np.int32), np.zeros((8, 8), np.float16)):
        with pytest.raises(TypeError):
            ac.set_potential(bad)
    for bad in (np.zeros((8, 8, 3), np.uint8), np.zeros((2, 8, 8, 3), np.float32), np.zeros((1, 8), np.uint8),
                np.zeros((8, 1), np.float32), np.zeros((3, 1, 9), np.uint8), np.zeros(8, np.uint8)):
        with pytest.raises(ValueError):
            ac.set_potential(bad)
    ac.clear_cache()
    for k in range(ActiveContour.max_cache_count + 5):
        ac._matrix(5, 1.0 + k)
    assert list(ac._Pinv_cache) == [(5, 1.0 + k) for k in range(5, ActiveContour.max_cache_count + 5)]
    if _hip.gpu_available():
        ac.set_potential(np.zeros((8, 8), np.uint8))
        assert ac.fx.shape == (8, 8)
    else:
        with pytest.raises(_hip.HipUnavailableError):
            ac.set_potential(np.zeros((8, 8), np.uint8))
        assert ac.fx is None
        from video import ops
        with pytest.raises(_hip.HipUnavailableError):
            ops.sobel5_f64(np.zeros((8, 8), np.float32))
