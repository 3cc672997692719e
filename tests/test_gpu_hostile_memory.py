"""GPU: every op on dirty device memory, with guarded buffer tails ("Hostile memory").

The `hostile` fixture switches the test fill mode on (video._hip.set_fill_mode): every host-layer buffer, every block
of library scratch and every plane a pipeline allocates starts out filled with 0xFF (int32 -1, all-ones label words,
NaN floats and doubles) or 0xA5 (large negative integers, finite non-zero floats), and every host-layer buffer has a
guarded tail that is checked when the buffer goes back.  Each test runs its op twice in a row -- the second call gets
recycled, refilled buffers and a cached, refilled scratch block -- and compares both results with np.array_equal
against the reference the family's own GPU test uses: the oracle, or the restatement of tests/golden/make_golden_*.py.
No tolerances.  Reads the oracle, the generators' restatements and the committed fixtures only.
"""
import importlib.util
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILLS = (0xFF, 0xA5)


def _generator(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(params=FILLS, ids=["fill_ff", "fill_a5"])
def hostile(request):
    """the test fill mode, on around one test; no guarded buffer leaks into another module's tests and no unguarded
    one into these"""
    from video import _hip, ops
    _hip.lib()
    ops.pool_clear()
    _hip.set_fill_mode(request.param)
    try:
        yield request.param
        found = _hip.check_guards()
    finally:
        _hip.set_fill_mode(-1)
        ops.pool_clear()
        _hip.check_guards()             # (what pool_clear's free() may still have recorded is not a later test's)
    assert found == [], found


_REFS = {}


def _ref(key, make):
    """a reference, computed once for both fill bytes and left unchanged"""
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


def _equal(got, want):
    """same structure (tuples / lists), dtype, shape and bytes"""
    if isinstance(want, (tuple, list)):
        assert isinstance(got, (tuple, list)) and len(got) == len(want), (type(got), len(want))
        for g, w in zip(got, want):
            _equal(g, w)
        return
    g, w = np.asarray(got), np.asarray(want)
    assert g.dtype == w.dtype and g.shape == w.shape, (g.dtype, w.dtype, g.shape, w.shape)
    assert np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes()      # (floats: the same bits)


def _twice(call, want, where=None):
    for run in (1, 2):
        try:
            _equal(call(), want)
        except AssertionError as e:
            raise AssertionError("%r, run %d: %s" % (where, run, e))


def _blob_clip(n, h, w, seed, nblobs=6, salt=0.0):
    rng = np.random.default_rng(seed)
    bg = np.clip(rng.normal(100, 10, (h, w)), 0, 255)
    yy, xx = np.mgrid[:h, :w]
    pos = rng.uniform(0, 1, (nblobs, 2)) * (w, h)
    vel = rng.uniform(-3, 3, (nblobs, 2))
    rad = rng.uniform(min(h, w) / 30 + 2, min(h, w) / 8 + 3, nblobs)
    out = np.empty((n, h, w), np.uint8)
    for t in range(n):
        f = bg + rng.normal(0, 4, (h, w))
        for (cx, cy), r in zip(pos + vel * t, rad):
            f[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] += 60
        if salt:
            f[rng.random((h, w)) < salt] = 255
        out[t] = np.clip(f, 0, 255).astype(np.uint8)
    return out


# ---------------------------------------------------------------------------------------------- the mode
def test_the_mode_is_on_in_the_library_and_in_the_host_layer(hostile):
    from video import _hip, ops
    L = _hip.lib()
    assert _hip.fill_mode() == hostile
    for bad in (-2, 256):
        assert L.va_test_hook_fill(bad) == -22 and b"va_test_hook_fill" in L.va_last_error()
    for recycled in (False, True):
        buf = ops._take(300)
        whole = np.empty(buf._alloc, np.uint8)
        _hip.check(L.va_memcpy_d2h(whole.ctypes.data, buf.ptr, whole.nbytes, None))
        _hip.check(L.va_stream_sync(None))
        assert whole.size == 512 + _hip.TAIL_BYTES and np.all(whole == hostile), recycled
        buf.upload(np.full(300, hostile ^ 0xFF, np.uint8))
        ops._give(buf)
    direct = _hip.DeviceBuffer(1000)
    assert direct.check_guard() is None and direct._alloc == 1000 + _hip.TAIL_BYTES
    direct.free()


# ---------------------------------------------------------------------------------------------- Gaussian
@pytest.mark.parametrize("sigma", [5.0, 1.0, 8.0])
@pytest.mark.parametrize("shape", [(3, 97, 208), (2, 10, 210)])
def test_gaussian_u8(hostile, oracle, shape, sigma):
    """the library's choice, the generic two-pass kernels, the dot4/dot2 kernel (rows of whole 16-byte vectors only)
    and the reference-era tap rule"""
    from video import ops
    im = _ref(("gu8_in", shape), lambda: np.random.default_rng(shape[2]).integers(0, 256, shape, dtype=np.uint8))
    ref = _ref(("gu8", shape, sigma), lambda: oracle.gaussian_u8(im, sigma))
    ref3 = _ref(("gu8cv3", shape, sigma), lambda: oracle.gaussian_u8(im, sigma, tap_rule="cv3"))
    impls = (None, "generic") + (("valu",) if shape[2] % 16 == 0 else ())
    for impl in impls:
        _twice(lambda: ops.gaussian_blur(im, sigma, implementation=impl), ref, impl)
    _twice(lambda: ops.gaussian_blur(im, sigma, tap_rule="cv3"), ref3, "cv3")


@pytest.mark.parametrize("sigma", [5.0, 1.0, 8.0])
def test_gaussian_u8_planes_path(hostile, oracle, sigma):
    from video import ops
    shape = (2, 33, 70, 3)
    im = _ref(("gpl_in",), lambda: np.random.default_rng(70).integers(0, 256, shape, dtype=np.uint8))
    for rule in ("cv4", "cv3"):
        ref = _ref(("gpl", sigma, rule), lambda: oracle.gaussian_u8(im, sigma, tap_rule=rule))
        _twice(lambda: ops.gaussian_blur(im, sigma, color=True, tap_rule=rule), ref, rule)
    ref = _ref(("gpl", sigma, "cv4"), None)
    _twice(lambda: ops.gaussian_blur(im, sigma, color=True, implementation="generic"), ref, "generic")


@pytest.mark.parametrize("generic", [0, 3])
def test_gaussian_f32(hostile, oracle, generic):
    """sigma = 2: radius 8, which has unrolled row and column kernels; generic = 3 runs both passes in the
    runtime-radius kernels instead"""
    from video import _hip, ops
    f = _ref(("gf32_in",), lambda: (np.random.default_rng(8).random((2, 97, 208), dtype=np.float32) * 2 - 0.5))
    ref = _ref(("gf32",), lambda: oracle.gaussian_f32(f, 2.0))
    _hip.check(_hip.lib().va_test_hook_gaussian_f32(generic))
    try:
        _twice(lambda: ops.gaussian_blur(f, 2.0), ref)
    finally:
        _hip.check(_hip.lib().va_test_hook_gaussian_f32(0))


# ------------------------------------------------------------------ background models, temporal statistics
def _bg_frames(dtype):
    rng = np.random.default_rng(22)
    if dtype == np.float32:
        return rng.random((5, 33, 70), dtype=np.float32)
    return rng.integers(0, 256, (5, 33, 70), dtype=np.uint8)


@pytest.mark.parametrize("mode,dtype", [("mean", np.uint8), ("ema", np.uint8), ("ema", np.float32),
                                        ("static", np.uint8)])
def test_background_models(hostile, oracle, mode, dtype):
    """va_bg_update, five frames folded in over two calls"""
    from video import ops
    fr = _ref(("bg_in", dtype), lambda: _bg_frames(dtype))
    static = _ref(("bg_static",), lambda: np.random.default_rng(23).random((33, 70)) * 255)

    def reference():
        if mode == "mean":
            return oracle.bg_mean_u8(fr)
        if mode == "static":
            return oracle.bg_static_u8(fr, static), static
        return (oracle.bg_ema_f32 if dtype == np.float32 else oracle.bg_ema_u8)(fr, rate=0.05)
    rd, rs = _ref(("bg", mode, dtype), reference)

    def call():
        m = ops.BackgroundModel(fr.shape[1:], mode, rate=0.05, dtype=dtype,
                                background=static if mode == "static" else None)
        try:
            d = np.concatenate([m.process(fr[:2]), m.process(fr[2:])])
            return d, m.state
        finally:
            m._state.free()             # the model owns its state
    _twice(call, (rd, rs.astype(np.float32) if mode == "ema" else rs))


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float32, np.float64])
def test_temporal_statistics(hostile, oracle, dtype):
    """va_mean_any, va_welford_any and va_welford_u8, split over two calls.  float64 frames, which the oracle's C
    restatement does not take, against the literal NumPy arithmetic of measure_mean / measure_mean_std"""
    from video import ops
    assert set(ops.TEMPORAL_DTYPES) == {np.dtype(t) for t in (np.uint8, np.int16, np.float32, np.float64)}

    def frames():
        rng = np.random.default_rng(17)
        if dtype == np.uint8:
            return rng.integers(0, 256, (5, 33, 70)).astype(np.uint8)
        if dtype == np.int16:
            return rng.integers(-255, 256, (5, 33, 70)).astype(np.int16)
        return rng.normal(0.4, 0.3, (5, 33, 70)).astype(dtype)
    fr = _ref(("tmp_in", dtype), frames)

    def reference():
        if dtype != np.float64:
            return oracle.mean_any(fr), oracle.welford_any(fr)
        mean = oracle.measure_mean_numpy(fr)
        wm, m2 = np.zeros(fr.shape[1:]), np.zeros(fr.shape[1:])
        for n, frame in enumerate(fr):
            delta = frame - wm
            wm = wm + delta / (n + 1)
            m2 = m2 + delta * (frame - wm)
        return mean, (wm, m2)
    mean, (wm, m2) = _ref(("tmp", dtype), reference)
    if dtype == np.uint8:
        _equal(oracle.welford_u8(fr), (wm, m2))

    def welford():
        a, b = ops.welford(fr[:2])
        return ops.welford(fr[2:], a, b, 2)
    _twice(lambda: ops.running_mean(fr[3:], ops.running_mean(fr[:3]), 3), mean)
    _twice(welford, (wm, m2))


# ------------------------------------------------------------------------------- pointwise and small ops
def _small(dtype=np.uint8, seed=31, channels=None):
    rng = np.random.default_rng(seed)
    shape = (2, 33, 70) + ((channels,) if channels else ())
    if np.dtype(dtype) == np.uint8:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    return (rng.random(shape) * 200).astype(dtype)


def test_pointwise(hostile, oracle):
    """threshold, mono mean, both normalizes, time difference, va_prepare_u8"""
    from video import _hip, ops
    a, b, col = _small(), _small(seed=32), _small(seed=33, channels=3)
    f = (_small(np.float32, seed=34) / 200).astype(np.float32)
    _twice(lambda: ops.threshold(a, 100), oracle.threshold_u8(a, 100))
    _twice(lambda: ops.threshold(a, 20, 1), oracle.threshold_u8(a, 20, 1))
    _twice(lambda: ops.mono_mean(col), oracle.mono_mean_u8(col))
    _twice(lambda: ops.time_difference(a, b), oracle.time_difference_u8(a, b))
    alpha = 255 / 170.0
    norm = ((np.clip(a.astype(np.float64), 30, 200) - 30) * alpha + 0).astype(np.int64).astype(np.uint8)
    _twice(lambda: ops.normalize(a, 30, 200, alpha, 0), norm)
    _twice(lambda: ops.normalize_any(a, 30, 200, alpha, 0, np.uint8), norm)
    for target in (np.float32, np.float64):
        want = ((np.clip(a.astype(np.float64), 30, 200) - 30) * (1.0 / 170.0) + 0).astype(target)
        _twice(lambda: ops.normalize_any(a, 30, 200, 1.0 / 170.0, 0, target), want, target)
    want = ((np.clip(f.astype(np.float64), 0.25, 0.75) - 0.25) * 510.0 + 0).astype(np.int64).astype(np.uint8)
    _twice(lambda: ops.normalize_any(f, 0.25, 0.75, 510.0, 0, np.uint8), want, "f32 -> u8")

    # crop (left 3, top 2, 64 x 30: the rows start at odd addresses), channel mean, normalize: one pass
    crop = col[:, 2:32, 3:67].astype(np.float64)
    mono = (crop.sum(-1) / 3.0).astype(np.uint8)
    want = ((np.clip(mono.astype(np.float64), 30, 200) - 30) * alpha).astype(np.int64).astype(np.uint8)

    def prepare():
        with ops._Lease() as d:
            src, dst = d.upload(col), d.take(want.size)
            _hip.check(_hip.lib().va_prepare_u8(src.ptr, dst.ptr, 2, 33, 70, 3, 3, 2, 64, 30, 3, 1, 30.0, 200.0, alpha,
                                                0.0, None))
            return dst.download(want.shape, np.uint8)
    _twice(prepare, want, "prepare")


@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.float64])
def test_rot90(hostile, dtype):
    """element sizes 1, 4 and 8"""
    from video import ops
    a = _small(dtype, seed=35)
    for k in (1, 2, 3):
        _twice(lambda: ops.rot90(a, k), np.rot90(a, k, axes=(1, 2)), k)


@pytest.fixture(scope="module")
def noise_reference():
    """the seeded stream with the mode off (module scope: made before any `hostile` of the tests that use it)"""
    from video import _hip, ops
    _hip.lib()
    assert _hip.fill_mode() == -1
    return {np.dtype(t): ops.gaussian_noise((2, 33, 70), t, 10.0, 3.0, seed=11, first_index=5)
            for t in (np.uint8, np.float32, np.float64)}


@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.float64])
def test_gaussian_noise(noise_reference, hostile, dtype):
    from video import ops
    want = noise_reference[np.dtype(dtype)]
    assert len(np.unique(want)) > 10
    _twice(lambda: ops.gaussian_noise((2, 33, 70), dtype, 10.0, 3.0, seed=11, first_index=5), want)


def _peak_images():
    rng = np.random.default_rng(71)
    u8 = (rng.integers(0, 256, (2, 33, 70)) // 32 * 32).astype(np.uint8)           # plateaus
    u8[1] = rng.integers(0, 6, (33, 70), dtype=np.uint8) * rng.integers(0, 2, (33, 70), dtype=np.uint8)
    f32 = rng.normal(0, 1, (2, 33, 70)).astype(np.float32)
    f32[1, 10:14, 20:26] = 2.5
    f32[1][f32[1] < 0] = 0
    return u8, f32


def test_detect_peaks(hostile, oracle):
    from video import ops
    for stack in _ref(("peaks_in",), _peak_images):
        for img in stack:
            for plateaus in (True, False):
                want = _ref(("peaks", img.tobytes(), plateaus), lambda: oracle.detect_peaks(img, plateaus))
                assert want.any()
                _twice(lambda: ops.detect_peaks(img, plateaus), want, (img.dtype, plateaus))


def test_image_statistics(hostile, oracle):
    """integer priors: every window sum is exact.  The box kernel (LDS tiles) and the ellipse (row prefixes)"""
    from video import ops
    u8 = _small(seed=77)
    f32 = (_small(np.float32, seed=78) - 50).astype(np.float32)
    for stack in (u8, f32):
        for img in stack:
            for kernel, ksize, prior, excl in (("box", 3, 128, False), ("ellipse", 4, 0, True), ("box", 9, 0, True)):
                want = _ref(("stats", img.tobytes(), kernel, ksize),
                            lambda: tuple(oracle.image_statistics(img, kernel, ksize, prior, excl)))
                _twice(lambda: ops.image_statistics(img, kernel, ksize, prior, excl), want, (img.dtype, kernel, ksize))
                _twice(lambda: ops.image_statistics(img, kernel, ksize, prior, excl, ret_var=False), want[0])


# ------------------------------------------------------------------------------------------------ resize
@pytest.mark.parametrize("mode", ["nearest", "linear", "cubic", "area", "lanczos"])
def test_resize(hostile, oracle, mode):
    from video import ops
    u8 = _ref(("rs_u8",), lambda: np.random.default_rng(91).integers(0, 256, (2, 37, 53), dtype=np.uint8))
    f32 = _ref(("rs_f32",), lambda: np.random.default_rng(92).random((2, 37, 53), dtype=np.float32))
    for size in ((23, 71), (74, 40)):
        _twice(lambda: ops.resize(u8, size, mode), _ref(("rs", "u8", mode, size), lambda: oracle.resize_u8(u8, size, mode)),
               ("u8", size))
        _twice(lambda: ops.resize(f32, size, mode),
               _ref(("rs", "f32", mode, size), lambda: oracle.resize_f32(f32, size, mode)), ("f32", size))


# -------------------------------------------------------------------------------------------- morphology
@pytest.mark.parametrize("shape", [(2, 33, 70), (1, 8, 210)])
def test_morphology_bytes_and_bits(hostile, oracle, shape):
    from video import ops
    rng = np.random.default_rng(shape[2])
    g = rng.integers(0, 256, shape, dtype=np.uint8)
    b = ((rng.random(shape) < 0.45) * 255).astype(np.uint8)
    for op, o in (("erode", oracle.ERODE), ("dilate", oracle.DILATE)):
        for sh, so in (("rect", oracle.RECT), ("cross", oracle.CROSS), ("ellipse", oracle.ELLIPSE)):
            for k in (3, 5):
                where = (op, sh, k)
                _twice(lambda: ops.morph(g, op, sh, k), _ref(("mo", shape, where), lambda: oracle.morph_u8(g, o, so, k)),
                       where)
                _twice(lambda: ops.morph(b, op, sh, k, implementation="bits"),
                       _ref(("mob", shape, where), lambda: oracle.morph_u8(b, o, so, k)), where + ("bits",))


# --------------------------------------------------------------------------------------------- labelling
PAINT_MODES = {"default": (0, 0), "chip-wide": (1, 0), "run-table": (2, 0), "sparse": (3, 0), "staged": (4, 0),
               "large-frame": (2, 7)}


@pytest.fixture(params=sorted(PAINT_MODES))
def paint_mode(request):
    from video import _hip
    path, lds_runs = PAINT_MODES[request.param]
    _hip.check(_hip.lib().va_test_hook_labelling(path, lds_runs))
    yield request.param
    _hip.check(_hip.lib().va_test_hook_labelling(0, 0))


def _label_masks(shape):
    """random frames of density 0.5; the last two frames of the stack are all zero and all one"""
    n, h, w = shape
    m = (np.random.default_rng(w).random((n + 2, h, w)) < 0.5).astype(np.uint8)
    m[n] = 0
    m[n + 1] = 1
    return m


def _label_reference(oracle, masks, conn):
    labels, counts = oracle.label_batch(masks, conn)
    stats = [oracle.region_stats(labels[f], int(counts[f])) for f in range(len(masks))]
    largest = []
    for f in range(len(masks)):
        if counts[f]:
            largest.append(oracle.get_largest_region(masks[f], ret_area=True, connectivity=conn))
        else:
            largest.append(None)
    return labels, counts, stats, largest


@pytest.mark.parametrize("shape", [(3, 33, 70), (1, 10, 208), (1, 8, 2112)])
def test_labelling(hostile, oracle, shape, paint_mode):
    """labels, counts, va_moments_i64, va_largest_region"""
    from video import ops
    masks = _ref(("lab_in", shape), lambda: _label_masks(shape))
    for conn in (4, 8):
        labels, counts, stats, largest = _ref(("lab", shape, conn), lambda: _label_reference(oracle, masks, conn))
        ml = int(counts.max())
        _twice(lambda: ops.label(masks, conn), (labels, counts), conn)

        def moments():
            return [ops.region_stats(labels[f], ml)[:int(counts[f]), :14] for f in range(len(masks))]
        _twice(moments, [s[:, :14] for s in stats], conn)
        for f in range(len(masks)):
            if largest[f] is None:
                _twice(lambda: ops.largest_region(masks[f], conn)[1:], (0, 0), (conn, f))
                continue
            region, area = largest[f]
            for run in (1, 2):
                got, garea, gcount = ops.largest_region(masks[f], conn)
                assert np.array_equal(got, region.astype(bool)) and garea == area and gcount == counts[f], (conn, f, run)


@pytest.mark.parametrize("shape", [(3, 33, 70), (1, 10, 208), (1, 8, 2112)])
def test_largest_contour_and_contour_moments(hostile, oracle, shape, paint_mode):
    """va_largest_contour, va_contour_moments (on the device's points and on uploaded ones) and
    va_contour_moments_ragged (find_contours(moments=True))"""
    from video import ops
    masks = _ref(("lab_in", shape), lambda: _label_masks(shape))

    def reference():
        out = []
        for m in masks:
            if not m.any():
                out.append(None)
                continue
            contour, area = oracle.get_contour_from_largest_region(m, ret_area=True)
            pts = np.asarray(contour, np.int32).reshape(-1, 2)
            mom = oracle.contour_moments(pts)
            out.append((pts, area, np.array([mom[k] for k in oracle.MOMENT_KEYS[:10]])))
        return out
    ref = _ref(("lc", shape), reference)
    for f, m in enumerate(masks):
        if ref[f] is None:
            continue
        pts, area, mom = ref[f]
        for run in (1, 2):
            gp, ga, _, gm = ops.largest_contour(m, moments=True)
            assert np.array_equal(gp, pts) and ga == area, (f, run)
            assert gm.tobytes() == mom.tobytes(), (f, run)
            assert ops.contour_moments(pts).tobytes() == mom.tobytes(), (f, run)
    for run in (1, 2):
        contours, moments = ops.find_contours(masks, moments=True)
        for f in range(len(masks)):
            assert len(contours[f]) == len(moments[f])
            for c, gm in zip(contours[f], moments[f]):
                mom = oracle.contour_moments(c.reshape(-1, 2))
                assert gm.tobytes() == np.array([mom[k] for k in oracle.MOMENT_KEYS[:10]]).tobytes(), (f, run)


# ---------------------------------------------------------------------------------- contours and skeletons
CG = _generator("make_golden_contours")
SG = _generator("make_golden_skeleton_graph")


def _same_lists(got, ref):
    assert len(got) == len(ref)
    for a, b in zip(got, ref):
        assert a.dtype == np.int32 and a.shape == b.shape and np.array_equal(a, b)


def test_find_contours(hostile, oracle):
    """two blob frames and a salt-noise frame, with the per-contour records"""
    from video import ops
    stack = _ref(("fc_in",), lambda: np.concatenate([CG.blob_stack((2, 33, 70), seed=5),
                                                     CG.random_mask(7, 33, 70, 0.1)[None]]))
    ref = _ref(("fc",), lambda: [oracle.find_contours_external_simple(m) for m in stack])
    assert all(len(r) > 1 for r in ref) and len(ref[2]) > 50
    for run in (1, 2):
        got, info = ops.find_contours(stack, ret_info=True)
        for f in range(len(stack)):
            _same_lists(got[f], ref[f])
            assert info[f]["area"].tolist() == [oracle.contour_area(c) for c in ref[f]], (f, run)
        _same_lists(ops.find_contours(stack[2]), ref[2])


def _same_graph(got, want, name):
    nodes, edges, lengths, curves = want
    assert np.array_equal(np.c_[got.nodes["x"], got.nodes["y"], got.nodes["degree"], got.nodes["pixels"]].reshape(-1, 4),
                          nodes), name
    assert np.array_equal(np.c_[got.edges["node_a"], got.edges["node_b"], got.edges["npoints"]].reshape(-1, 3),
                          edges), name
    assert got.edges["length"].dtype == np.float64 and np.array_equal(got.edges["length"], lengths), name
    assert len(got.curves) == len(curves), name
    for c, w in zip(got.curves, curves):
        assert c.dtype == np.int32 and np.array_equal(c, w), name


def test_skeleton_graphs(hostile):
    """the ragged batch of the hand cases, the fixture skeletons and the border items; a stack of two frames"""
    from video import ops

    def ragged():
        cases = list(SG.all_cases().items()) + SG.border_items()
        return [n for n, _ in cases], [m for _, m in cases], [SG.skeleton_graph(m) for _, m in cases]
    names, imgs, want = _ref(("sg",), ragged)

    def frames():
        T = SG.thinning()
        stack = np.stack([T.guo_hall(T.blob(900 + k, 33, 70, 3.0, -0.2))[0] for k in range(2)])
        return stack, [SG.skeleton_graph(f) for f in stack]
    stack, want_stack = _ref(("sg_stack",), frames)
    assert all(len(w[0]) > 2 for w in want_stack)
    for run in (1, 2):
        for name, g, w in zip(names, ops.skeleton_graphs(imgs), want):
            _same_graph(g, w, (name, run))
        for k, (g, w) in enumerate(zip(ops.skeleton_graphs(stack), want_stack)):
            _same_graph(g, w, ("frame", k, run))


# ---------------------------------------------------------------------------------------------- geodesic
def test_geodesic_maps_paths_and_farthest_points(hostile):
    """the three smallest masks of the fixture, among those of a hundred pixels or more, that have a path"""
    from video.analysis import regions
    geo = np.load(os.path.join(ROOT, "tests", "golden", "geodesic_v1.npz"), allow_pickle=False)
    names = [n for n in geo["names"] if tuple(geo[n + "/path_end"]) != (-1, -1) and geo[n + "/mask"].any()
             and geo[n + "/mask"].size >= 100]
    names = sorted(names, key=lambda n: geo[n + "/mask"].size)[:3]
    assert len(names) == 3
    for name in names:
        mask = geo[name + "/mask"]
        starts = [tuple(p) for p in geo[name + "/starts"]]
        e = geo[name + "/ends"]
        ends = [tuple(p) for p in e] if len(e) else None
        end = tuple(int(v) for v in geo[name + "/path_end"])
        fg = (mask != 0).astype(np.uint8)
        p1 = tuple(int(v) for v in geo[name + "/fp_p1_in"])
        for run in (1, 2):
            m = mask.astype(np.int32)
            regions.make_distance_map(m, starts, ends)
            assert np.array_equal(m, geo[name + "/map"]), (name, run)
            assert np.array_equal(regions.shortest_path_in_distance_map(geo[name + "/map"], end),
                                  geo[name + "/path"]), (name, run)
            assert np.array_equal(np.array(regions.get_farthest_points(fg, p1)), geo[name + "/fp"]), (name, run)
            assert np.array_equal(regions.get_farthest_points(fg, p1, ret_path=True), geo[name + "/fp_path"]), (name, run)


# ------------------------------------------------------------------------------------------ optical flow
OG = _generator("make_golden_optflow")
# the smallest pair stacks of test_gpu_optflow.RANDOM_CASES (with their seeds): a tiny frame, the winsize-5 branch, and
# one with several pyramid levels
FLOW_CASES = [(3, 2, 5, 7, {}), (4, 2, 9, 11, dict(winsize=5)), (0, 2, 40, 50, {})]


@pytest.mark.parametrize("case", range(len(FLOW_CASES)))
def test_farneback_flow(hostile, case):
    from video import ops
    seed, n, h, w, extra = FLOW_CASES[case]
    params = OG.params_of(extra)
    frames = _ref(("of_in", case), lambda: OG.texture_frames(n, h, w, 100 + seed, step=((seed % 3) - 1, 1 + seed % 2)))
    want = _ref(("of", case), lambda: tuple(OG.optical_flow(frames, **params)))
    _twice(lambda: ops.optical_flow_farneback(frames, ret_flow=True, **params), want)


# ----------------------------------------------------------------------------------- snakes and polygons
AG = _generator("make_golden_active_contour")
PG = _generator("make_golden_polygon")


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_sobel5(hostile):
    from video import ops
    for dt in (np.uint8, np.float32):
        x = np.stack([AG.sobel_input(33, 70, dt, salt=s) for s in (1, 2)])
        want = _ref(("sobel", dt), lambda: AG.sobel5(x))
        for run in (1, 2):
            gx, gy = ops.sobel5_f64(x)
            assert _bits_equal(gx, want[0]) and _bits_equal(gy, want[1]), (dt, run)
            assert ops.sobel5_f64(x, dx=False)[0] is None and _bits_equal(ops.sobel5_f64(x, dx=False)[1], want[1])


def _snake_restated(ac, curve, gx, gy, anchor_x=None, anchor_y=None):
    from video.analysis import curves
    pts = curves.make_curve_equidistant(curve)
    ds = curves.curve_length(pts) / (len(pts) - 1)
    flags, vals = ac._anchors(curve, pts, anchor_x, anchor_y)
    p, it, tv, _ = AG.snake(gx, gy, pts, ac.get_evolution_matrix(len(pts), ds), ac.gamma,
                            ac.residual_tolerance * ac.gamma, ac.max_iterations, flags, vals)
    return p, it, tv


@pytest.mark.parametrize("npoints", [128, 129])
def test_active_contour(hostile, npoints):
    """128 points are the last that keep the matrix in LDS; 129 read it from global memory"""
    from video.analysis.active_contour import ActiveContour
    for run in (1, 2):
        ac = ActiveContour(closed_loop=True, **AG.PARAMS["ref"])
        ac.max_iterations = 50
        ac.residual_tolerance = 1
        ac.set_potential(AG.potential("f32"))
        want = _ref(("grad",), lambda: AG.gradients(AG.potential("f32"), ac.blur_radius))
        assert _bits_equal(ac.fx, want[0]) and _bits_equal(ac.fy, want[1]), run
        curve = AG.ellipse_curve(npoints, True)
        got = ac.find_contour(curve)
        p, it, tv = _ref(("snake", npoints), lambda: _snake_restated(ac, curve, ac.fx, ac.fy))
        assert _bits_equal(got, p) and ac.info["iteration_count"] == it, (npoints, run)
        assert _bits_equal(ac.info["total_variation"], tv), (npoints, run)


GRAD_SHAPES = ((3, 3), (2, 13), (10, 2), (1, 7), (5, 5), (6, 9), (27, 82), (37, 53))


@pytest.mark.parametrize("sigma", [0.0, 1.0])
def test_ragged_gradients(hostile, sigma):
    """va_potential_gradients_ragged; the planes it returns are buffers of their own, checked when they are freed"""
    from video import ops
    items = [AG.sobel_input(h, w, np.float32, salt=7 * k + 1) for k, (h, w) in enumerate(GRAD_SHAPES)]
    want = _ref(("rg", sigma), lambda: [AG.gradients(p, sigma) for p in items])
    total = sum(p.size for p in items)
    for run in (1, 2):
        fx, fy, shapes, offsets = ops.potential_gradients_ragged(items, sigma)
        try:
            flats = [b.download((total,), np.float64) for b in (fx, fy)]
        finally:
            fx.free()
            fy.free()
        for k, ((h, w), o) in enumerate(zip(shapes.tolist(), offsets.tolist())):
            for flat, plane in zip(flats, want[k]):
                assert _bits_equal(flat[o:o + h * w].reshape(h, w), plane), (sigma, k, run)


@pytest.mark.parametrize("closed", [False, True])
def test_ragged_snakes(hostile, closed):
    """va_active_contour_ragged over two potentials of different shapes, anchors included"""
    from video.analysis.active_contour import ActiveContour
    pots = [AG.potential("f32")[:60, :80].copy(), AG.potential("f32_soft")[20:65, 30:130].copy()]
    half = lambda c: c * 0.5                                   # noqa: E731
    jobs = [(half(AG.ellipse_curve(40, closed)), 0, None, None),
            (AG.ellipse_curve(64, closed) - [30.0, 20.0], 1, None, None),
            (half(AG.ellipse_curve(5, closed)), 0, None, None)]
    if not closed:
        jobs += [(half(AG.ellipse_curve(48, False)), 0, [0, 47], [0, 47]),
                 (AG.ellipse_curve(64, False) - [30.0, 20.0], 1, [0, 20, 63], None)]
    for run in (1, 2):
        ac = ActiveContour(closed_loop=closed, **AG.PARAMS["ref"])
        ac.set_potential(pots)
        got = ac.find_contours([j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs], [j[3] for j in jobs])
        its, tvs = ac.info["iteration_count"].copy(), ac.info["total_variation"].copy()
        grads = _ref(("rs_grad",), lambda: [AG.gradients(p, ac.blur_radius) for p in pots])
        for k, (curve, item, ax, ay) in enumerate(jobs):
            assert _bits_equal(ac.fx[item], grads[item][0]) and _bits_equal(ac.fy[item], grads[item][1]), (k, run)
            p, it, tv = _ref(("rs", closed, k),
                             lambda: _snake_restated(ac, curve, grads[item][0], grads[item][1], ax, ay))
            assert _bits_equal(got[k], p) and its[k] == it and _bits_equal(tvs[k], tv), (closed, k, run)


def test_fill_poly_and_distance_transform(hostile):
    from video import ops
    from video.analysis.shapes import Polygon
    names = list(PG.FILL_POLYS)
    boxes = [PG.bounding_rect(PG.FILL_POLYS[n], 1) for n in names]
    contours = [np.asarray(PG.FILL_POLYS[n], np.float64).astype(np.int64) for n in names]       # as Polygon.get_mask
    masks = _ref(("fp",), lambda: [PG.fill_poly(c, b) for c, b in zip(contours, boxes)])
    dts = _ref(("dt",), lambda: [PG.distance_transform(m) for m in masks])
    for run in (1, 2):
        for dtype in (np.uint8, np.int32):
            got = ops.fill_polys(contours, boxes, dtype)
            for n, g, w in zip(names, got, masks):
                assert g.dtype == dtype and np.array_equal(g, w), (n, dtype, run)
        for n, g, w in zip(names, ops.distance_transform(masks), dts):
            assert g.dtype == np.float32 and np.array_equal(g.view(np.uint32), w.view(np.uint32)), (n, run)
        assert np.array_equal(Polygon(PG.FILL_POLYS[names[0]]).get_mask(1), masks[0])


def test_centerlines_optimized(hostile):
    """one batched get_centerlines_optimized of four small polygons"""
    from video.analysis.shapes import Polygon, get_centerlines_optimized
    params = dict(alpha=10., beta=100., gamma=0.01, spacing=5, max_iterations=60)
    names = ["hexagon", "l_shape", "u_shape", "tiny"]
    endpoints = [[[5, 3], [29, 33]] if n == "l_shape" else None for n in names]
    want = _ref(("cl",), lambda: [PG.optimized(PG.FILL_POLYS[n], endpoints=ep, **params)
                                  for n, ep in zip(names, endpoints)])
    for run in (1, 2):
        got = get_centerlines_optimized([Polygon(PG.FILL_POLYS[n]) for n in names], endpoints=endpoints, **params)
        for n, g, w in zip(names, got, want):
            assert _bits_equal(g, w), (n, run)


# ---------------------------------------------------------------------------------------------- thinning
TG = _generator("make_golden_thinning")


def test_guo_hall_thinning_ragged(hostile):
    """masks in LDS: every eighth mask of the resident batch, the widest included"""
    from video import ops

    def batch():
        cases = TG.resident_batch()
        words = [ops._thin_words(m.shape) for _, m in cases]
        pick = sorted(set(range(0, len(cases), 8)) | {int(np.argmax(words))})
        masks = [cases[k][1] for k in pick]
        want = [TG.guo_hall(m) for m in masks]
        return masks, [s for s, _ in want], [i for _, i in want]
    masks, skels, iters = _ref(("th",), batch)
    assert max(ops._thin_words(m.shape) for m in masks) == ops.THIN_RESIDENT_MAX_WORDS
    for run in (1, 2):
        got, it = ops.guo_hall_thinning(masks, implementation="resident", ret_iterations=True)
        assert it.tolist() == iters, run
        for k, (g, w) in enumerate(zip(got, skels)):
            assert g.dtype == np.uint8 and np.array_equal(g, w), (k, run)


def test_guo_hall_thinning_tiled_stack(hostile):
    """the tiled path with the caller's scratch, on frames that are no multiple of the tile or of a word"""
    from video import ops
    stack = _ref(("tt_in",), lambda: np.stack([TG.blob(810 + k, 97, 208, 2.5 + 1.5 * k, -0.2) for k in range(2)]))
    want = _ref(("tt",), lambda: [TG.guo_hall(f) for f in stack])
    for run in (1, 2):
        got, it = ops.guo_hall_thinning(stack, implementation="tiled", ret_iterations=True)
        assert np.array_equal(got, np.stack([s for s, _ in want])) and it.tolist() == [i for _, i in want], run


def test_mask_thinning(hostile, oracle):
    from video import ops
    yy, xx = np.mgrid[:33, :70]
    blob = (((xx - 30) / 25.0) ** 2 + ((yy - 16) / 9.0) ** 2 <= 1) | (abs(xx - 55) + abs(yy - 14) < 11)
    for m in (blob.astype(np.uint8) * 255, blob[:32, :68].astype(np.uint8)):
        want = _ref(("mt", m.shape), lambda: oracle.mask_thinning(m))
        for run in (1, 2):
            skel, it = ops.mask_thinning(m)
            assert it == want[1] and np.array_equal(skel, want[0]), (m.shape, run)


# ------------------------------------------------------------------------------------------------- warps
LG = _generator("make_golden_line_scan")


def _rotation(angle_deg, src_shape, dst_shape):
    a = math.radians(angle_deg)
    c, s = math.cos(a), math.sin(a)
    cx, cy = (src_shape[1] - 1) / 2.0, (src_shape[0] - 1) / 2.0
    dx, dy = (dst_shape[1] - 1) / 2.0, (dst_shape[0] - 1) / 2.0
    return np.array([[c, s, dx - c * cx - s * cy], [-s, c, dy + s * cx - c * cy]])


def test_line_scans_and_warp_affine(hostile):
    from video import ops
    frames = LG.gpu_frames()
    cases = LG.gpu_batch()
    cases = cases[::max(len(cases) // 40, 1)][:40]
    assert len(cases) == 40
    strips = _ref(("ls",), lambda: [LG.line_scan_strip(frames[f], p1, p2, hw)[1] for f, p1, p2, hw in cases])
    fidx = np.array([c[0] for c in cases])
    p1, p2 = np.array([c[1] for c in cases], np.float64), np.array([c[2] for c in cases], np.float64)
    hw = np.array([c[3] for c in cases], np.float64)
    sizes = [(1, 1), (1, 70), (70, 1), (33, 65)]
    mats = [_rotation(10.0 * k + 7, frames.shape[1:], s) for k, s in enumerate(sizes)]
    widx = [0, 1, 2, 1]
    warped = _ref(("wa",), lambda: [LG.warp_affine(frames[f], M, (s[1], s[0])) for f, M, s in zip(widx, mats, sizes)])
    for run in (1, 2):
        profiles, sums = ops.line_scans(frames, p1, p2, hw, frame_index=fidx, ret_sums=True)
        for k, (prof, sm, strip) in enumerate(zip(profiles, sums, strips)):
            assert np.array_equal(sm, strip.sum(axis=0, dtype=np.int64)), (k, run)
            assert prof.dtype == np.float64 and np.array_equal(prof, strip.mean(axis=0)), (k, run)
        got = ops.warp_affine(frames, mats, sizes, frame_index=widx)
        for k, (g, w) in enumerate(zip(got, warped)):
            assert g.dtype == np.uint8 and g.shape == sizes[k] and np.array_equal(g, w), (k, run)
        got = ops.warp_affine(frames, [LG.invert(M) for M in mats], sizes, frame_index=widx, inverse=True)
        for k, (g, w) in enumerate(zip(got, warped)):
            assert np.array_equal(g, w), (k, run)


# -------------------------------------------------------------------------------------------- the engine
CLOSE5 = (("dilate", "rect", 5), ("erode", "rect", 5))
MAX_LABELS = 32


def _engine(**kw):
    from video.engine import FrameEngine
    return FrameEngine(**kw)


def _chain_reference(oracle, clip, background, conn, sigma=5.0, thresh=20):
    """filtered, mask, labels, counts, per-frame statistics and the background state of the full chain"""
    if background == "mean":
        diff, state = oracle.bg_mean_u8(clip)
    else:
        diff, state = oracle.bg_ema_u8(clip, rate=0.05)
    blur = oracle.gaussian_u8(diff, sigma)
    m = oracle.threshold_u8(blur, thresh)
    m = oracle.morph_u8(oracle.morph_u8(m, oracle.DILATE, oracle.RECT, 5), oracle.ERODE, oracle.RECT, 5)
    labels, counts = oracle.label_batch(m, conn)
    stats = [oracle.region_stats(labels[f], int(counts[f])) for f in range(len(clip))]
    return dict(filtered=blur, mask=m, labels=labels, counts=counts, stats=stats, state=state)


def _check_outputs(out, ref, want, where):
    assert set(out) == set(want) | ({"counts"} if "stats" in want else set()), where
    for k in ("filtered", "mask", "labels", "counts"):
        if k in out:
            assert out[k].dtype == ref[k].dtype and np.array_equal(out[k], ref[k]), where + (k,)
    if "stats" in out:
        for f, rs in enumerate(ref["stats"]):
            c = min(int(ref["counts"][f]), MAX_LABELS)
            assert np.array_equal(out["stats"][f, :c, :14], rs[:c, :14]), where + ("stats", f)


# every combination that selects another instantiation of the labelling and paint kernels
WANTS = (("labels", "counts"), ("counts",), ("stats",), ("filtered", "mask", "labels"), ("mask",),
         ("filtered", "mask", "labels", "counts", "stats"))


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("background", ["mean", "ema"])
@pytest.mark.parametrize("shape", [(3, 97, 208), (2, 10, 210)])
def test_engine_full_chain(hostile, oracle, shape, background, conn):
    """background model, sigma = 5, threshold, 5 x 5 close, labelling: the engine is created with the mode on, so
    that its planes are filled; every run starts from a fresh background model and gives the oracle's outputs"""
    n, h, w = shape
    clip = _ref(("eng_in", shape), lambda: _blob_clip(n, h, w, seed=h + w, salt=0.01))
    ref = _ref(("eng", shape, background, conn), lambda: _chain_reference(oracle, clip, background, conn))
    assert ref["counts"].max() >= 1
    eng = _engine(size=(w, h), max_batch=n, background=background, bg_rate=0.05, sigma=5.0, thresh=20, morphology=CLOSE5,
                  connectivity=conn, max_labels=MAX_LABELS)
    try:
        for run in (1, 2):
            for want in WANTS:
                eng.set_background(None, 0)
                _check_outputs(eng.run(clip, want=want), ref, want, (want, run))
                state, n_seen = eng.get_background()
                assert n_seen == n and np.array_equal(state, ref["state"]), (want, run)
        # the label image written on the engine's own stream, from the planes va_pipeline_overlap allocates
        eng.overlap(True)
        for run in (1, 2, 3):
            eng.set_background(None, 0)
            _check_outputs(eng.run(clip, want=WANTS[-1]), ref, WANTS[-1], ("overlap", run))
    finally:
        eng.close()


def test_engine_forced_valu_gaussian(hostile, oracle):
    from video import _hip
    shape = n, h, w = (3, 97, 208)
    clip = _ref(("eng_in", shape), lambda: _blob_clip(n, h, w, seed=h + w, salt=0.01))
    ref = _ref(("eng", shape, "mean", 4), lambda: _chain_reference(oracle, clip, "mean", 4))
    _hip.check(_hip.lib().va_test_hook_gaussian_u8(1))
    try:
        eng = _engine(size=(w, h), max_batch=n, background="mean", sigma=5.0, thresh=20, morphology=CLOSE5,
                      connectivity=4, max_labels=MAX_LABELS)
    finally:
        _hip.check(_hip.lib().va_test_hook_gaussian_u8(0))
    try:
        assert "mfma" not in eng.description.lower()
        for run in (1, 2):
            for want in (WANTS[-1], ("mask",), ("counts",)):
                eng.set_background(None, 0)
                _check_outputs(eng.run(clip, want=want), ref, want, (want, run))
    finally:
        eng.close()


def test_engine_float32_chain(hostile, oracle):
    """the chain of cfg#5 (float32 x 3 channels, EMA background, sigma = 9) on two small frames, split over two runs"""
    rng = np.random.default_rng(5)
    clip = _ref(("f32_in",), lambda: (rng.random((4, 33, 70, 3), dtype=np.float32) * 0.5 + 0.25))

    def reference():
        d, bg = oracle.bg_ema_f32(clip, rate=0.02)
        return oracle.gaussian_f32(d, 9.0), bg
    blur, bg = _ref(("f32",), reference)
    eng = _engine(size=(70, 33), channels=3, dtype=np.float32, max_batch=2, background="ema", bg_rate=0.02, sigma=9.0)
    try:
        for run in (1, 2):
            eng.set_background(None, 0)
            got = np.concatenate([eng.run(clip[:2], want=("filtered",))["filtered"],
                                  eng.run(clip[2:], want=("filtered",))["filtered"]])
            assert np.array_equal(got.view(np.uint32), blur.view(np.uint32)), run
            assert np.array_equal(eng.get_background()[0].view(np.uint32), bg.view(np.uint32)), run
    finally:
        eng.close()


def test_streamed_engine(hostile, oracle):
    """uploads, chain and downloads on three streams, three batches through two slots"""
    from video.streaming import StreamedEngine
    shape = n, h, w = (6, 33, 70)
    clip = _ref(("eng_in", shape), lambda: _blob_clip(n, h, w, seed=h + w, salt=0.01))
    ref = _ref(("eng", shape, "mean", 4), lambda: _chain_reference(oracle, clip, "mean", 4))
    want = ("mask", "labels", "counts", "stats")
    for run in (1, 2):
        eng = _engine(size=(w, h), max_batch=2, background="mean", sigma=5.0, thresh=20, morphology=CLOSE5,
                      connectivity=4, max_labels=MAX_LABELS)
        try:
            results = []
            with StreamedEngine(eng, want=want, slots=2) as s:
                for a in range(0, n, 2):
                    results += s.submit(clip[a:a + 2], tag=a)
                results += s.drain()
            assert [r["tag"] for r in results] == [0, 2, 4]
            out = {k: np.concatenate([r[k] for r in results]) for k in want}
            _check_outputs(out, ref, want, ("streamed", run))
        finally:
            eng.close()
