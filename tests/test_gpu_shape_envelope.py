"""GPU: every core and first-tier op at the edges of its shape envelope ("Shape envelope").

The contract: a call either returns the oracle's bytes or is refused with VA_ERR_INVALID before anything is enqueued,
with a message that names the limit include/videoanalysis_hip.h states.  REFUSED is the whole list of refusals these
shapes may meet; every other case here must compute, and VA_ERR_HIP or a different byte fails the test.

  group A  degenerate frames: 1 x 1 ... 64 x 2, three frames each (one random, one all zero, one all 255), and n = 0
  group B  the smallest shapes on either side of each gate in the launch code, at n = 2 and n = 9 (a partial group of
           eight frames)
  group C  more than 65535 frames, rows, columns or ragged items in one call: what the kernels put into
           gridDim.y / gridDim.z, and what makes the library split a launch or take another kernel

Groups A and B run twice: plainly, and in the test fill mode (tests/test_gpu_hostile_memory.py) with byte 0xA5, where
a write behind a tiny frame's buffer lands in a guarded tail instead of the slack of a size class.

Which case guards which launch code:
  the pieces of edge_labels_kernel (va_contours.hip)   test_c_contours_of_more_than_65535_frames (va_find_contours) and
                                                       test_c_farthest_points_of_more_than_65535_frames
  the pieces of the float row pass                     test_c_gaussian[65537x4x8]: sigma 1 takes the fused kernels
  the periodic reflection of col_sym_f32_kernel        test_b_gaussian_f32_gates, heights 1, 2 and r - 1, hook 0
  the periodic reflection of col_march_f32_kernel      the same heights under hook bit 0 (the runtime-radius columns)

Every comparison is on dtype, shape and bytes (floats: the same bits).  A batch of more than 64 frames repeats 64
distinct ones, and the reference of an op that treats frames independently is computed for those and repeated.
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, PERIOD = -22, 64
CLOSE5 = (("dilate", "rect", 5), ("erode", "rect", 5))

DEGENERATE = [(1, 1), (1, 2), (2, 1), (1, 5), (5, 1), (2, 2), (3, 3), (3, 4), (4, 3), (1, 33), (33, 1), (2, 64), (64, 2)]
GROUP_A = [(3,) + hw for hw in DEGENERATE] + [(0, 4, 4)]
GROUP_C = [(65537, 2, 4), (65537, 4, 8), (1, 65537, 4), (1, 65537, 1), (1, 2, 65540), (1, 1, 65537)]

# (entry point, case) -> (words of the VA_ERR_INVALID message, words of include/videoanalysis_hip.h): the limit
REFUSED = {
    ("va_optical_flow_farneback", "n = 65537"): ("more than 65535 frames", "at most 65535 frames"),
    ("va_optical_flow_farneback", "h = 65537"): ("more than 65535 rows", "at most 65535 rows"),
    ("va_guo_hall_thinning_u8", "n = 65537"): ("at most 65535 frames", "1 .. 65535 frames"),
    ("va_guo_hall_thinning_u8", "h = VA_THIN_MAX_ROWS + 1"): ("at most 2097120", "at most VA_THIN_MAX_ROWS rows"),
    ("va_resize_u8", "dst_h = 65536"): ("more than 65535 rows", "dst_h <= 65535"),
    ("va_resize_f32", "dst_h = 65536"): ("more than 65535 rows", "dst_h <= 65535"),
}


def _sibling(name, *where):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", *where, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _ids(shape):
    return "x".join(str(v) for v in shape)


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def ops():
    from video import _hip, ops as _ops
    _hip.lib()          # raises HipUnavailableError (loudly) if the extension/GPU is missing
    return _ops


@pytest.fixture(params=["plain", "fill_a5"])
def memory(request):
    """groups A and B: once as it is, once in the test fill mode with byte 0xA5 (the `hostile` fixture of
    tests/test_gpu_hostile_memory.py), every guarded tail checked afterwards"""
    from video import _hip, ops
    _hip.lib()
    if request.param == "plain":
        yield request.param
        return
    ops.pool_clear()
    _hip.set_fill_mode(0xA5)
    try:
        yield request.param
        found = _hip.check_guards()
    finally:
        _hip.set_fill_mode(-1)
        ops.pool_clear()
        _hip.check_guards()             # (what pool_clear's free() may still have recorded is not a later test's)
    assert found == [], found


@pytest.fixture(params=["frame-lds", "frame-staged", "frame-large", "chip-wide"])
def ccl_mode(request):
    """the four labelling code paths of tests/test_gpu_parity.py (va_test_hook_labelling)"""
    from video import _hip
    path, lds_runs = {"frame-lds": (2, 0), "frame-staged": (4, 0), "frame-large": (2, 7),
                      "chip-wide": (1, 0)}[request.param]
    _hip.check(_hip.lib().va_test_hook_labelling(path, lds_runs))
    yield request.param
    _hip.check(_hip.lib().va_test_hook_labelling(0, 0))


def _engine(**kw):
    from video import _hip
    from video.engine import FrameEngine
    _hip.lib()
    return FrameEngine(**kw)


_REFS = {}


def _ref(key, make):
    """a reference, computed once for every run that needs it and left unchanged"""
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


# ------------------------------------------------------------------------------------------------ helpers
def _equal(got, want, where=None):
    """same structure (tuples / lists), dtype, shape and bytes"""
    if isinstance(want, (tuple, list)):
        assert isinstance(got, (tuple, list)) and len(got) == len(want), (where, type(got), len(want))
        for g, w in zip(got, want):
            _equal(g, w, where)
        return
    g, w = np.asarray(got), np.asarray(want)
    assert g.dtype == w.dtype and g.shape == w.shape, (where, g.dtype, w.dtype, g.shape, w.shape)
    if g.tobytes() != w.tobytes():
        bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
        raise AssertionError("%r: %d of %d elements differ, first at %s" % (where, bad.size, g.size, bad[:4]))


def _tile(base, n):
    """n frames (or per-frame results) out of the distinct ones of `base`"""
    return base if len(base) == n else base[np.arange(n) % len(base)]


def _base(n, h, w, c=None, seed=0):
    """the distinct uint8 frames of an n-frame batch: seeded random; frame 1 all zero, frame 2 all 255"""
    k = min(n, PERIOD)
    a = np.random.default_rng(seed + 1000 * h + w).integers(0, 256, (k, h, w) + ((c,) if c else ()), dtype=np.uint8)
    if k >= 3:
        a[1], a[2] = 0, 255
    return a


def _base_f32(n, h, w, c=None, seed=0):
    """float32 frames in [-1, 3): frame 1 is the constant -1, frame 2 the constant 2.984375"""
    return (_base(n, h, w, c, seed).astype(np.float32) / 64 - 1).astype(np.float32)


def _base_masks(n, h, w, seed=0):
    """0 / 1 masks of density one half; frame 1 all zero, frame 2 all one"""
    k = min(n, PERIOD)
    m = (np.random.default_rng(seed + 1000 * h + w).random((k, h, w)) < 0.5).astype(np.uint8)
    if k >= 3:
        m[1], m[2] = 0, 1
    return m


def _per_frame(fn, base, dtype=None):
    """fn(frame) for every distinct frame, stacked"""
    out = [fn(f) for f in base]
    if not out:
        return np.zeros(base.shape, dtype or base.dtype)
    return np.stack(out)


def _refused(entry, case, call):
    """the call is refused with VA_ERR_INVALID, its message names the limit, and the header states it"""
    from video import _hip
    message, stated = REFUSED[(entry, case)]
    with pytest.raises(_hip.HipError) as err:
        call()
    assert err.value.code == INVALID, (entry, case, err.value)
    assert message in str(err.value), (entry, case, err.value)
    text = open(os.path.join(ROOT, "include", "videoanalysis_hip.h")).read()
    header = " ".join(t for t in text.split() if t != "*")          # (comment continuation marks)
    at = header.index(" " + entry + "(")
    section = header[max(0, at - 4000):at]                          # the comment in front of the prototype
    assert stated in section, (entry, case, stated)


def _f32_radius(oracle, sigma):
    return oracle.gauss_ksize(sigma, False) // 2


# ======================================================================================= the ops, at one shape
# Each check takes (n, h, w), builds the batch from its distinct frames and compares with the oracle.  Groups A and C
# run them all; `light` keeps the parameter sets of group C to what chooses another launch path.
def check_gaussian_u8(ops, oracle, n, h, w, sigmas=(1.0, 5.0, 8.0)):
    base = _base(n, h, w)
    a = _tile(base, n)
    for sigma in sigmas:
        want = _tile(_ref(("gu8", n, h, w, sigma), lambda: oracle.gaussian_u8(base, sigma)), n)
        r = oracle.gauss_ksize(sigma, True) // 2
        valu = w >= 32 and h >= 32 and w % 16 == 0 and (r <= 16 or (w >= 64 and h >= 64))    # va_gauss_fused.hip:366
        for impl in (None, "generic") + (("valu",) if valu else ()):
            _equal(ops.gaussian_blur(a, sigma, implementation=impl), want, ("gaussian u8", sigma, impl))


def check_gaussian_f32(ops, oracle, n, h, w, sigmas=(1.0, 2.0, 9.0), channels=(None, 3)):
    for c in channels:
        base = _base_f32(n, h, w, c)
        a = _tile(base, n)
        for sigma in sigmas:
            want = _tile(_ref(("gf32", n, h, w, c, sigma), lambda: oracle.gaussian_f32(base, sigma)), n)
            _equal(ops.gaussian_blur(a, sigma, color=bool(c)), want, ("gaussian f32", sigma, c))


def check_background(ops, oracle, n, h, w):
    """the temporal ops fold the frames in order: their references take the whole batch"""
    a, f = _tile(_base(n, h, w), n), _tile(_base_f32(n, h, w), n)
    static = np.random.default_rng(h + w).random((h, w)) * 255
    key = ("bg", n, h, w)
    _equal(ops.running_mean(a), _ref(key + ("mean",), lambda: oracle.mean_any(a)), "running_mean")
    _equal(ops.running_mean(f), _ref(key + ("mean f32",), lambda: oracle.mean_any(f)), "running_mean f32")
    _equal(ops.welford(a), _ref(key + ("welford",), lambda: oracle.welford_u8(a)), "welford")
    _equal(ops.welford(f), _ref(key + ("welford f32",), lambda: oracle.welford_any(f)), "welford f32")
    models = (("mean", np.uint8, a, lambda: oracle.bg_mean_u8(a)),
              ("ema", np.uint8, a, lambda: oracle.bg_ema_u8(a, rate=0.05)),
              ("ema", np.float32, f, lambda: oracle.bg_ema_f32(f, rate=0.05)),
              ("static", np.uint8, a, lambda: (oracle.bg_static_u8(a, static), static)))
    for mode, dtype, frames, reference in models:
        diff, state = _ref(key + (mode, dtype), reference)
        m = ops.BackgroundModel((h, w), mode, rate=0.05, dtype=dtype, background=static if mode == "static" else None)
        try:
            _equal((m.process(frames), m.state), (diff, state.astype(np.float32) if mode == "ema" else state),
                   ("va_bg_update", mode, dtype))
        finally:
            m._state.free()             # the model owns its state
    if n >= 2:
        _equal(ops.time_difference(a[1:], a[:-1]), oracle.time_difference_u8(a[1:], a[:-1]), "time_difference")


def check_pointwise(ops, oracle, n, h, w):
    a, col = _tile(_base(n, h, w), n), _tile(_base(n, h, w, 3, seed=5), n)
    _equal(ops.threshold(a, 100), oracle.threshold_u8(a, 100), "threshold")
    _equal(ops.mono_mean(col), oracle.mono_mean_u8(col), "mono_mean")
    alpha = 255 / 170.0
    norm = ((np.clip(a.astype(np.float64), 30, 200) - 30) * alpha + 0).astype(np.int64).astype(np.uint8)
    _equal(ops.normalize(a, 30, 200, alpha, 0), norm, "normalize")
    f = _tile(_base_f32(n, h, w), n)
    for k in (1, 2, 3):
        _equal(ops.rot90(a, k), np.ascontiguousarray(np.rot90(a, k, axes=(1, 2))), ("rot90 u8", k))
        _equal(ops.rot90(f, k), np.ascontiguousarray(np.rot90(f, k, axes=(1, 2))), ("rot90 f32", k))
    _equal(ops.rot90(col, 1, color=True), np.ascontiguousarray(np.rot90(col, 1, axes=(1, 2))), "rot90 3 bytes")


MORPH_ELEMENTS = (("rect", 3), ("rect", 5), ("rect", 31), ("ellipse", 9), ("cross", 5))


def check_morph(ops, oracle, n, h, w, elements=MORPH_ELEMENTS):
    gray, binary = _base(n, h, w), _base_masks(n, h, w) * np.uint8(255)
    codes = {"rect": oracle.RECT, "ellipse": oracle.ELLIPSE, "cross": oracle.CROSS}
    for op, o in (("dilate", oracle.DILATE), ("erode", oracle.ERODE)):
        for shape, k in elements:
            want = _tile(_ref(("mo", n, h, w, op, shape, k), lambda: oracle.morph_u8(gray, o, codes[shape], k)), n)
            _equal(ops.morph(_tile(gray, n), op, shape, k), want, ("morph", op, shape, k))
            want = _tile(_ref(("mob", n, h, w, op, shape, k), lambda: oracle.morph_u8(binary, o, codes[shape], k)), n)
            _equal(ops.morph(_tile(binary, n), op, shape, k, implementation="bits"), want, ("bits", op, shape, k))


def check_label_and_stats(ops, oracle, n, h, w):
    """va_label_i32 and va_moments_i64 on the whole batch"""
    base = _base_masks(n, h, w)
    masks = _tile(base, n)
    for conn in (4, 8):
        labels, counts = _ref(("lab", n, h, w, conn), lambda: oracle.label_batch(base, conn))
        _equal(ops.label(masks, conn), (_tile(labels, n), _tile(counts, n)), ("label", conn))
        ml = int(counts.max(initial=0))
        stats = _ref(("st", n, h, w, conn), lambda: [oracle.region_stats(labels[f], int(counts[f])) for f in range(len(base))])
        got = ops.region_stats(_tile(labels, n), ml)
        assert got.dtype == np.int64 and got.shape == (n, max(ml, 1), 16)
        want = np.zeros((len(base), max(ml, 1), 14), np.int64)
        used = np.zeros((len(base), max(ml, 1)), bool)
        for f, s in enumerate(stats):
            want[f, :len(s)], used[f, :len(s)] = s[:, :14], True
        _equal(got[:, :, :14][_tile(used, n)], _tile(want, n)[_tile(used, n)], ("region_stats", conn))


def _contour_reference(oracle, m):
    """(points, area, ten moments, 8-connected components) of the largest contour; points None for an empty mask"""
    count = oracle.label(m, 8)[1]
    if not m.any():
        return None, 0.0, None, count
    contour, area = oracle.get_contour_from_largest_region(m, ret_area=True)
    pts = np.asarray(contour, np.int32).reshape(-1, 2)
    mom = oracle.contour_moments(pts)
    return pts, area, np.array([mom[k] for k in oracle.MOMENT_KEYS[:10]]), count


def check_single_mask_ops(ops, oracle, n, h, w):
    """the ops whose wrapper takes one mask: largest_region, largest_contour, contour_moments, mask_thinning"""
    base = _base_masks(n, h, w)
    for f, m in enumerate(base):
        for conn in (4, 8):
            got = ops.largest_region(m, conn)
            count = oracle.label(m, conn)[1]
            if count == 0:
                assert not got[0].any() and got[1:] == (0, 0), (f, conn)
                continue
            region, area = _ref(("lr", n, h, w, f, conn),
                                lambda: oracle.get_largest_region(m, ret_area=True, connectivity=conn))
            _equal(got[0], region.astype(bool), ("largest_region", f, conn))
            assert got[1:] == (area, count), (f, conn, got[1:])
        pts, area, mom, count = _ref(("lc", n, h, w, f), lambda: _contour_reference(oracle, m))
        gp, ga, gc, gm = ops.largest_contour(m, moments=True)
        assert gc == count, ("largest_contour", f, gc, count)
        if pts is None:
            assert gp.shape == (0, 2), (f, gp.shape)
        else:
            _equal(gp, pts, ("largest_contour", f))
            assert ga == area, (f, ga, area)
            _equal(gm, mom, ("contour moments on the device's points", f))
            _equal(ops.contour_moments(pts), mom, ("contour_moments", f))
        skel, it = _ref(("thin", n, h, w, f), lambda: oracle.mask_thinning(m))
        gs, gi = ops.mask_thinning(m)
        _equal(gs, skel, ("mask_thinning", f))
        assert gi == it, ("mask_thinning iterations", f, gi, it)


def check_find_contours(ops, oracle, n, h, w):
    base = _base_masks(n, h, w)
    ref = _ref(("fc", n, h, w), lambda: [oracle.find_contours_external_simple(m) for m in base])
    areas = _ref(("fca", n, h, w), lambda: [[oracle.contour_area(c) for c in r] for r in ref])
    got, info = ops.find_contours(_tile(base, n), ret_info=True) if n else ([], [])
    assert len(got) == n
    for f in range(n):
        want = ref[f % PERIOD]
        assert len(got[f]) == len(want), ("find_contours", f, len(got[f]), len(want))
        for a, b in zip(got[f], want):
            assert a.dtype == np.int32 and a.shape == b.shape and np.array_equal(a, b), ("find_contours", f)
        assert info[f]["area"].tolist() == areas[f % PERIOD], ("contour areas", f)
    if n:
        _equal(ops.find_contours(base[0]), ref[0], "one mask")


def _float_equal(got, want, where):
    """bits, except where the reference is NaN: the mean and variance of a window of one sample are 0/0, whose sign
    and payload IEEE 754 leaves to the implementation -- there the result must be a NaN, whichever"""
    g, w = np.asarray(got), np.asarray(want)
    assert g.dtype == w.dtype and g.shape == w.shape, (where, g.dtype, w.dtype, g.shape, w.shape)
    nan = np.isnan(w)
    assert np.isnan(g[nan]).all(), where
    _equal(g[~nan], w[~nan], where)


STATS_CASES = [(kernel, ksize) for kernel in ("box", "ellipse") for ksize in (0, 2, 5)]


def check_peaks_and_statistics(ops, oracle, n, h, w, stats_cases=STATS_CASES):
    """the stencils whose wrapper takes one image; integer priors, so that every window sum is exact"""
    for base in (_base(n, h, w) // 32 * 32, np.floor(_base_f32(n, h, w) * 8).astype(np.float32)):
        for f, img in enumerate(base):
            for plateaus in (True, False):
                want = _ref(("pk", n, h, w, str(base.dtype), f, plateaus), lambda: oracle.detect_peaks(img, plateaus))
                _equal(ops.detect_peaks(img, plateaus), want, ("detect_peaks", base.dtype, f, plateaus))
            for kernel, ksize in stats_cases:
                with np.errstate(all="ignore"):
                    want = _ref(("is", n, h, w, str(base.dtype), f, kernel, ksize),
                                lambda: oracle.image_statistics(img, kernel, ksize, 3, False))
                got = ops.image_statistics(img, kernel, ksize, 3)
                for g, wv, what in zip(got, want, ("mean", "variance")):
                    _float_equal(g, wv, ("image_statistics", what, base.dtype, f, kernel, ksize))


RESIZE_MODES = ("nearest", "linear", "cubic", "area", "lanczos")


def check_resize(ops, oracle, n, h, w, modes=RESIZE_MODES):
    bu, bf = _base(n, h, w), _base_f32(n, h, w)
    for mode in modes:
        for size in ((1, 1), (2, 3)):               # (width, height): frames of 1 x 1 and of 3 x 2
            want = _tile(_ref(("rs", n, h, w, mode, size), lambda: oracle.resize_u8(bu, size, mode)), n)
            _equal(ops.resize(_tile(bu, n), size, mode), want, ("resize u8", mode, size))
            want = _tile(_ref(("rsf", n, h, w, mode, size), lambda: oracle.resize_f32(bf, size, mode)), n)
            _equal(ops.resize(_tile(bf, n), size, mode), want, ("resize f32", mode, size))


# ============================================================================================== group A
@pytest.mark.parametrize("shape", GROUP_A, ids=_ids)
def test_a_gaussian(memory, ops, oracle, shape):
    check_gaussian_u8(ops, oracle, *shape)
    check_gaussian_f32(ops, oracle, *shape)


def test_a_background_and_pointwise(memory, ops, oracle):
    for shape in GROUP_A:
        check_background(ops, oracle, *shape)
        check_pointwise(ops, oracle, *shape)


def test_a_morphology(memory, ops, oracle):
    for shape in GROUP_A:
        check_morph(ops, oracle, *shape)


def test_a_labelling_and_contours(memory, ops, oracle, ccl_mode):
    for shape in GROUP_A:
        check_label_and_stats(ops, oracle, *shape)
        check_single_mask_ops(ops, oracle, *shape)
        check_find_contours(ops, oracle, *shape)


def test_a_peaks_and_statistics(memory, ops, oracle):
    for shape in GROUP_A:
        check_peaks_and_statistics(ops, oracle, *shape)


def test_a_resize(memory, ops, oracle):
    for shape in GROUP_A:
        check_resize(ops, oracle, *shape)


def test_a_empty_batches_have_the_right_shape_and_dtype(ops):
    """n = 0: nothing to compute, and what comes back is an empty array of the batch's shape"""
    a, f = np.zeros((0, 4, 4), np.uint8), np.zeros((0, 4, 4), np.float32)
    for got, shape, dtype in ((ops.gaussian_blur(a, 2.0), (0, 4, 4), np.uint8),
                              (ops.gaussian_blur(f, 2.0), (0, 4, 4), np.float32),
                              (ops.gaussian_blur(np.zeros((0, 4, 4, 3), np.float32), 2.0, color=True), (0, 4, 4, 3), np.float32),
                              (ops.threshold(a, 3), (0, 4, 4), np.uint8),
                              (ops.normalize(a, 0, 1, 1, 0), (0, 4, 4), np.uint8),
                              (ops.mono_mean(np.zeros((0, 4, 4, 3), np.uint8)), (0, 4, 4), np.uint8),
                              (ops.rot90(np.zeros((0, 4, 5), np.uint8)), (0, 5, 4), np.uint8),
                              (ops.morph(a, "dilate"), (0, 4, 4), np.uint8),
                              (ops.morph(a, "erode", implementation="bits"), (0, 4, 4), np.uint8),
                              (ops.resize(a, (2, 3)), (0, 3, 2), np.uint8),
                              (ops.resize(f, (2, 3), "area"), (0, 3, 2), np.float32),
                              (ops.label(a)[0], (0, 4, 4), np.int32), (ops.label(a)[1], (0,), np.int32),
                              (ops.region_stats(np.zeros((0, 4, 4), np.int32), 2), (0, 2, 16), np.int64),
                              (ops.running_mean(a), (4, 4), np.float64), (ops.welford(a)[1], (4, 4), np.float64)):
        assert got.shape == shape and got.dtype == dtype, (got.shape, got.dtype, shape, dtype)
    assert ops.find_contours(a) == []


# ============================================================================================== group B
# 8-bit Gaussian: gauss_fused_supported (w < 32 || h < 32 || w % 16) and gauss_mfma_supported (w < 64 || h < 32 ||
# w % 16); widths that are no multiple of 16 take the planes path where the padded plane passes the second gate
U8_GATES = [(31, 64), (32, 64), (33, 64), (32, 48), (32, 32), (31, 32), (32, 16), (40, 63), (40, 65), (40, 80)]


@pytest.mark.parametrize("sigma", [1.0, 5.0, 8.0])
def test_b_gaussian_u8_gates(memory, ops, oracle, sigma):
    paint = _sibling("test_gpu_gauss_paint_paths")
    r = oracle.gauss_ksize(sigma, True) // 2
    for h, w in U8_GATES:
        for n in (2, 9):
            check_gaussian_u8(ops, oracle, n, h, w, sigmas=(sigma,))
            if w >= 64 and h >= 32 and w % 16 == 0 and r <= 16:       # gauss_mfma_supported: the engine's choice
                paint._check_three_outputs(oracle, _base(n, h, w), sigma, 127, maxval=200)


@pytest.mark.parametrize("sigma", [1.0, 2.0, 9.0])
def test_b_gaussian_f32_gates(memory, ops, oracle, sigma):
    """plan_rows / plan_rows_is (w <= r, w c % 4) and the column kernels: heights below the radius reflect more than
    once, 121 and 129 cross the 120-row and 128-row steps of the 15- and 16-row kernels.  Once as the library chooses,
    once under each bit of va_test_hook_gaussian_f32 (runtime-radius columns, runtime-radius rows)"""
    from video import _hip
    r = _f32_radius(oracle, sigma)
    assert r == 4 * sigma
    for hook in (0, 1, 2):
        _hip.check(_hip.lib().va_test_hook_gaussian_f32(hook))
        try:
            for w in (r, r + 1, r + 3, r + 4):
                for h in (1, 2, r - 1, r, r + 1, 121, 129):
                    for n in (2, 9):
                        check_gaussian_f32(ops, oracle, n, h, w, sigmas=(sigma,))
        finally:
            _hip.check(_hip.lib().va_test_hook_gaussian_f32(0))


B_WIDTHS, B_HEIGHTS = (31, 32, 33, 63, 64, 65), (1, 4, 5)      # mask-word boundaries, w % 4 != 0; rows of the x4 kernels


def test_b_morphology_at_the_word_boundaries(memory, ops, oracle):
    for h in B_HEIGHTS:
        for w in B_WIDTHS:
            for n in (2, 9):
                check_morph(ops, oracle, n, h, w)


def test_b_labelling_at_the_word_boundaries(memory, ops, oracle, ccl_mode):
    for h in B_HEIGHTS:
        for w in B_WIDTHS:
            for n in (2, 9):
                check_label_and_stats(ops, oracle, n, h, w)
                check_find_contours(ops, oracle, n, h, w)


def _chain_clip(n, h, w):
    """a noisy background around 100 with blocks of 4 x 4 pixels raised by 100 in a third of the places"""
    rng = np.random.default_rng(100 * h + w + n)
    clip = rng.integers(90, 110, (n, h, w))
    marks = rng.random((n, (h + 3) // 4, (w + 3) // 4)) < 0.3
    clip += 100 * np.repeat(np.repeat(marks, 4, axis=1), 4, axis=2)[:, :h, :w]
    return clip.astype(np.uint8)


@pytest.mark.parametrize("size", [(1, 1), (5, 1), (1, 5), (3, 3), (33, 2), (64, 31), (63, 32), (64, 32)], ids=_ids)
def test_b_engine_full_chain(memory, oracle, size):
    """background mean, sigma 5, threshold, 5 x 5 closing, labels, counts and statistics against oracle.chain_u8"""
    h, w = size
    ml = 16
    for n in (2, 9):
        clip = _chain_clip(n, h, w)
        mask, labels, counts, mean = _ref(("chain", n, h, w),
                                          lambda: oracle.chain_u8(clip, 5.0, 20, morph_ksize=5, connectivity=4))
        eng = _engine(size=(w, h), max_batch=n, background="mean", sigma=5.0, thresh=20, morphology=CLOSE5,
                      connectivity=4, max_labels=ml)
        try:
            out = eng.run(clip, want=("mask", "labels", "counts", "stats"))
            state = eng.get_background()
        finally:
            eng.close()
        _equal((out["mask"], out["labels"], out["counts"]), (mask, labels, counts), ("chain", n))
        _equal(state[0], mean, ("background", n))
        assert state[1] == n
        for f in range(n):
            k = min(int(counts[f]), ml)
            _equal(out["stats"][f, :k, :14], oracle.region_stats(labels[f], int(counts[f]))[:k, :14], ("stats", n, f))


@pytest.mark.parametrize("sigma", [2.0, 9.0])
@pytest.mark.parametrize("shape", [(8, 8, 1), (12, 3, 3), (40, 37, 1)], ids=_ids)
def test_b_engine_f32_ema_and_blur(memory, oracle, shape, sigma):
    """float32 frames, EMA background and blur in one engine (the float references of tests/test_gpu_configs.py)"""
    h, w, c = shape
    rate = 0.3
    for n in (2, 9):
        full = (n, h, w, c) if c > 1 else (n, h, w)
        clip = (np.random.default_rng(n + w).random(full, dtype=np.float32) * 2 - 0.5).astype(np.float32)

        def reference():
            diff, bg = oracle.bg_ema_f32(clip.reshape(n, -1), rate=np.float32(rate))
            return oracle.gaussian_f32(diff.reshape(full), sigma), bg.reshape(full[1:])
        ref, bg = _ref(("f32 chain", n, shape, sigma), reference)
        eng = _engine(size=(w, h), channels=c, dtype=np.float32, max_batch=n, background="ema", bg_rate=rate, sigma=sigma)
        try:
            got = eng.run(clip, want=("filtered",))["filtered"]
            state, seen = eng.get_background()
        finally:
            eng.close()
        assert seen == n
        _equal(state, bg, ("state", n))
        _equal(got, ref, ("filtered", n))


# ============================================================================================== group C
@pytest.mark.parametrize("shape", GROUP_C, ids=_ids)
def test_c_gaussian(ops, oracle, shape):
    """sigma 1 at 65537 x 4 x 8 takes the fused float kernels, whose row pass counts frames in gridDim.y: the
    compile-time-radius kernel as the library chooses, the runtime-radius kernel under hook bit 1"""
    from video import _hip
    check_gaussian_u8(ops, oracle, *shape)
    check_gaussian_f32(ops, oracle, *shape, sigmas=(1.0, 2.0))
    _hip.check(_hip.lib().va_test_hook_gaussian_f32(2))
    try:
        check_gaussian_f32(ops, oracle, *shape, sigmas=(1.0,))
    finally:
        _hip.check(_hip.lib().va_test_hook_gaussian_f32(0))


@pytest.mark.parametrize("shape", GROUP_C, ids=_ids)
def test_c_background_pointwise_morphology_resize(ops, oracle, shape):
    check_background(ops, oracle, *shape)
    check_pointwise(ops, oracle, *shape)
    check_morph(ops, oracle, *shape)
    check_resize(ops, oracle, *shape)


@pytest.mark.parametrize("shape", GROUP_C, ids=_ids)
def test_c_labelling(ops, oracle, shape, ccl_mode):
    check_label_and_stats(ops, oracle, *shape)


@pytest.mark.parametrize("shape", GROUP_C, ids=_ids)
def test_c_contours_of_more_than_65535_frames(ops, oracle, shape):
    """va_find_contours on the batch: edge_labels_kernel counts frames in gridDim.y"""
    check_find_contours(ops, oracle, *shape)


def test_c_engines_with_more_than_65535_frames_in_a_batch(oracle):
    """FrameEngine with max_batch = 65537 on 4 x 8 frames: the full 8-bit chain, and float32 EMA + blur"""
    n, h, w = 65537, 4, 8
    clip = _tile(_chain_clip(PERIOD, h, w), n)
    mask, labels, counts, mean = oracle.chain_u8(clip, 5.0, 20, morph_ksize=5, connectivity=4)
    eng = _engine(size=(w, h), max_batch=n, background="mean", sigma=5.0, thresh=20, morphology=CLOSE5, connectivity=4)
    try:
        out = eng.run(clip, want=("mask", "labels", "counts"))
        state = eng.get_background()
    finally:
        eng.close()
    _equal((out["mask"], out["labels"], out["counts"]), (mask, labels, counts), "chain")
    _equal(state[0], mean, "background")
    assert state[1] == n
    f = _tile(_base_f32(n, h, w), n)
    diff, bg = oracle.bg_ema_f32(f.reshape(n, -1), rate=np.float32(0.3))
    ref = oracle.gaussian_f32(diff.reshape(f.shape), 1.0)
    eng = _engine(size=(w, h), dtype=np.float32, max_batch=n, background="ema", bg_rate=0.3, sigma=1.0)
    try:
        got = eng.run(f, want=("filtered",))["filtered"]
        state, seen = eng.get_background()
    finally:
        eng.close()
    assert seen == n
    _equal(state, bg.reshape(h, w), "state")
    _equal(got, ref, "filtered")


def _arc_length(contour):
    """cv2.arcLength(contour, closed=True): float32 differences and sqrt, summed in double from the closing segment
    on (tests/test_gpu_geodesic.py)"""
    pts = np.asarray(contour).reshape(-1, 2).astype(np.float32)
    per, prev = 0.0, pts[-1]
    for p in pts:
        d = p - prev
        per += float(np.sqrt(np.float32(d[0] * d[0] + d[1] * d[1])))
        prev = p
    return per


@pytest.mark.parametrize("shape", GROUP_C[:2], ids=_ids)
def test_c_farthest_points_of_more_than_65535_frames(ops, oracle, shape):
    """va_farthest_points without start points begins at the longest outer contour of each frame: the other caller of
    edge_labels_kernel.  Against the restatement of tests/golden/make_golden_geodesic.py"""
    G = _sibling("make_golden_geodesic", "golden")
    n, h, w = shape
    base = _base_masks(n, h, w)
    want = np.full((len(base), 2, 2), -1, np.int64)
    for f, m in enumerate(base):
        if m.any():
            c = max(oracle.find_contours_external_simple(m), key=_arc_length)
            want[f] = G.farthest_points(m, (int(c[0, 0, 0]), int(c[0, 0, 1])))
    p1, p2 = ops.farthest_points(_tile(base, n))
    some = _tile(base.reshape(len(base), -1).any(axis=1), n)
    _equal(p1, _tile(want[:, 0], n), "p1")
    _equal(p2[some], _tile(want[:, 1], n)[some], "p2")


@pytest.mark.parametrize("shape", [s for s in GROUP_C if s[0] == 1], ids=_ids)
def test_c_single_image_ops_on_long_frames(ops, oracle, shape):
    check_single_mask_ops(ops, oracle, *shape)
    check_peaks_and_statistics(ops, oracle, *shape, stats_cases=[("box", 2), ("ellipse", 5)])


@pytest.mark.parametrize("shape", [s for s in GROUP_C if s[0] > 1], ids=_ids)
def test_c_single_image_entry_points_on_many_frames(ops, oracle, shape):
    """the entry points whose wrapper takes one image, called on the whole batch: va_detect_peaks_*,
    va_image_statistics_*, va_largest_contour + va_contour_moments, va_moments_i64 + va_largest_region"""
    from video import _hip
    L, check = _hip.lib(), _hip.check
    n, h, w = shape
    for base in (_base(n, h, w) // 32 * 32, np.floor(_base_f32(n, h, w) * 8).astype(np.float32)):
        u8 = base.dtype == np.uint8
        stack = _tile(base, n)
        with ops._Lease() as d:
            src, dst, dm, dv = d.upload(stack), d.take(stack.size), d.take(stack.size * 8), d.take(stack.size * 8)
            for plateaus in (True, False):
                check((L.va_detect_peaks_u8 if u8 else L.va_detect_peaks_f32)(src.ptr, dst.ptr, n, h, w, int(plateaus), None))
                want = _per_frame(lambda img: oracle.detect_peaks(img, plateaus), base, bool)
                _equal(dst.download(stack.shape, np.uint8).astype(bool), _tile(want, n), ("peaks", base.dtype, plateaus))
            for kernel, ksize in (("box", 2), ("ellipse", 5)):
                check((L.va_image_statistics_u8 if u8 else L.va_image_statistics_f32)(
                    src.ptr, dm.ptr, dv.ptr, n, h, w, int(kernel == "ellipse"), ksize, 3.0, 0, None))
                mean = _per_frame(lambda img: oracle.image_statistics(img, kernel, ksize, 3, False)[0], base)
                var = _per_frame(lambda img: oracle.image_statistics(img, kernel, ksize, 3, False)[1], base)
                _equal(dm.download(stack.shape, np.float64), _tile(mean, n), ("mean", base.dtype, kernel))
                _equal(dv.download(stack.shape, np.float64), _tile(var, n), ("variance", base.dtype, kernel))
    base = _base_masks(n, h, w)
    masks = _tile(base, n)
    cap = h * w
    refs = [_contour_reference(oracle, m) for m in base]
    with ops._Lease() as d:
        ws_bytes = L.va_contour_workspace_bytes(n, h, w)
        src, ws, pts, npts, area, ncomp, mom = (d.upload(masks), d.take(ws_bytes), d.take(n * cap * 8), d.take(n * 4),
                                                d.take(n * 8), d.take(n * 4), d.take(n * 80))
        check(L.va_largest_contour(src.ptr, n, h, w, pts.ptr, cap, npts.ptr, area.ptr, ncomp.ptr, ws.ptr, ws_bytes, None))
        check(L.va_contour_moments(pts.ptr, npts.ptr, n, cap, 0, mom.ptr, None))
        gp, gn, ga, gc, gm = (pts.download((n, cap, 2), np.int32), npts.download((n,), np.int32),
                              area.download((n,), np.float64), ncomp.download((n,), np.int32),
                              mom.download((n, 10), np.float64))
    _equal(gc, _tile(np.array([r[3] for r in refs], np.int32), n), "components")
    _equal(gn, _tile(np.array([0 if r[0] is None else len(r[0]) for r in refs], np.int32), n), "points per contour")
    some = _tile(np.array([r[0] is not None for r in refs]), n)
    _equal(ga[some], _tile(np.array([r[1] for r in refs]), n)[some], "areas")
    _equal(gm[some], _tile(np.stack([np.zeros(10) if r[2] is None else r[2] for r in refs]), n)[some], "moments")
    want = np.zeros((len(base), cap, 2), np.int32)
    for f, r in enumerate(refs):
        if r[0] is not None:
            want[f, :len(r[0])] = r[0]
    kept = np.arange(cap)[None, :] < gn[:, None]
    _equal(gp[kept], _tile(want, n)[kept], "points")
    for conn in (4, 8):
        labels, counts = oracle.label_batch(base, conn)
        ml = int(counts.max())
        regions = [oracle.get_largest_region(m, ret_area=True, connectivity=conn) if c else None
                   for m, c in zip(base, counts)]
        with ops._Lease() as d:
            lab, cnt = ops._label(d, masks, n, h, w, conn)
            st, big, area, sel = d.take(n * ml * _hip.STATS_STRIDE * 8), d.take(n * 4), d.take(n * 8), d.take(masks.size)
            check(L.va_moments_i64(lab.ptr, n, h, w, ml, st.ptr, None))
            check(L.va_largest_region(lab.ptr, cnt.ptr, st.ptr, n, h, w, ml, big.ptr, area.ptr, sel.ptr, None))
            gb, ga, gs = big.download((n,), np.int32), area.download((n,), np.int64), sel.download(masks.shape, np.uint8)
        some = _tile(counts > 0, n)
        assert (gb[~some] == 0).all() and (gb[some] > 0).all(), conn
        _equal(ga[some], _tile(np.array([r[1] if r else 0 for r in regions], np.int64), n)[some], ("largest area", conn))
        want = np.stack([r[0].astype(np.uint8) if r else np.zeros((h, w), np.uint8) for r in regions])
        _equal(gs[some], _tile(want, n)[some], ("largest region", conn))


def _ragged_items():
    """64 distinct 3 x 3 masks (the centre set in all of them, so that none is empty) and which of them item k is"""
    rng = np.random.default_rng(33)
    items = (rng.random((PERIOD, 3, 3)) < 0.6).astype(np.uint8)
    items[:, 1, 1] = 1
    items[0], items[1] = 1, 0
    items[1, 1, 1] = 1
    return items, np.arange(65537) % PERIOD


def test_c_ragged_ops_with_more_than_65535_items(ops):
    """fill_polys, distance_transform, guo_hall_thinning, skeleton_graphs and line_scans put the item in gridDim.x:
    65537 items of 3 x 3 in one call, against the per-item restatements of tests/golden/make_golden_*.py"""
    PG, TG, SG, LG = (_sibling(name, "golden") for name in ("make_golden_polygon", "make_golden_thinning",
                                                            "make_golden_skeleton_graph", "make_golden_line_scan"))
    items, which = _ragged_items()
    batch = [items[k] for k in which]
    m = len(batch)

    want = [PG.distance_transform(a) for a in items]
    got = ops.distance_transform(batch)
    assert len(got) == m
    _equal(np.stack(got), np.stack(want)[which], "distance_transform")

    want = [TG.guo_hall(a)[0] for a in items]
    got = ops.guo_hall_thinning(batch)
    _equal(np.stack(got), np.stack(want).astype(np.uint8)[which], "guo_hall_thinning")
    _equal(ops.guo_hall_thinning(np.stack(batch), implementation="tiled"), np.stack(want).astype(np.uint8)[which],
           "guo_hall_thinning, tiled: the host layer sends pieces of 65535 frames")

    rng = np.random.default_rng(34)
    polys = [rng.integers(-1, 4, (3 + k % 3, 2)) for k in range(PERIOD)]
    boxes = [(0, 0, 3, 3)] * PERIOD
    want = np.stack([PG.fill_poly(c, b) for c, b in zip(polys, boxes)])
    got = ops.fill_polys([polys[k] for k in which], [boxes[k] for k in which])
    _equal(np.stack(got), want[which], "fill_polys")

    skeletons = [TG.guo_hall(a)[0] for a in items]
    want = [SG.skeleton_graph(s) for s in skeletons]
    got = ops.skeleton_graphs([skeletons[k].astype(np.uint8) for k in which])
    assert len(got) == m
    for k in list(range(0, m, 257)) + list(range(m - PERIOD, m)):           # every 257th item and the last 64: whole graphs
        nodes, edges, lengths, curves = want[which[k]]
        g = got[k]
        assert np.array_equal(np.c_[g.nodes["x"], g.nodes["y"], g.nodes["degree"], g.nodes["pixels"]].reshape(-1, 4), nodes), k
        assert np.array_equal(np.c_[g.edges["node_a"], g.edges["node_b"], g.edges["npoints"]].reshape(-1, 3), edges), k
        assert np.array_equal(g.edges["length"], lengths) and len(g.curves) == len(curves), k
        for a, b in zip(g.curves, curves):
            assert np.array_equal(a, b), k
    for k in range(m):                                                        # every item: the sizes of its graph
        nodes, edges = want[which[k]][:2]
        assert len(got[k].nodes) == len(nodes) and len(got[k].edges) == len(edges), k

    frames = np.random.default_rng(35).integers(0, 256, (PERIOD, 3, 3), dtype=np.uint8)
    p1, p2 = np.tile([[0.0, 1.0]], (m, 1)), np.tile([[2.0, 1.0]], (m, 1))
    want = np.stack([LG.line_scan(f, (0.0, 1.0), (2.0, 1.0), 1) for f in frames])
    got = ops.line_scans(frames, p1, p2, 1, frame_index=which.astype(np.int32))
    _equal(np.stack(got), want[which], "line_scans")


# ------------------------------------------------------------------------------------------- the refusals
def _optical_flow(ops, shape):
    return lambda: ops.optical_flow_farneback(np.zeros(shape, np.uint8))


def _thinning_abi(ops, n, h, w):
    """va_guo_hall_thinning_u8 itself (the host layer sends pieces and checks the rows before it calls); the shape
    is refused before any pointer is looked at"""
    from video import _hip

    def call():
        buf = ops._take(256)
        try:
            _hip.check(_hip.lib().va_guo_hall_thinning_u8(buf.ptr, buf.ptr, 256, buf.ptr, n, h, w, 0, 0, None, None, None))
        finally:
            ops._give(buf)
    return call


def _resize_abi(ops, dtype):
    """65536 target rows; the target buffer must come back as it was"""
    from video import _hip

    def call():
        src = np.arange(4, dtype=dtype).reshape(1, 2, 2)
        before = np.full((1, 65536, 1), 7, dtype)
        with ops._Lease() as d:
            s, t = d.upload(src), d.upload(before)
            fn = _hip.lib().va_resize_u8 if dtype == np.uint8 else _hip.lib().va_resize_f32
            try:
                _hip.check(fn(s.ptr, t.ptr, 1, 2, 2, 1, 65536, 1, 1, None))
            finally:
                _equal(t.download(before.shape, dtype), before, "the refused call's target")
    return call


def test_c_documented_refusals(ops, oracle):
    """every entry of REFUSED, and nothing else in this module, is refused"""
    calls = {
        ("va_optical_flow_farneback", "n = 65537"): _optical_flow(ops, (65537, 2, 4)),
        ("va_optical_flow_farneback", "h = 65537"): _optical_flow(ops, (2, 65537, 4)),
        ("va_guo_hall_thinning_u8", "n = 65537"): _thinning_abi(ops, 65537, 2, 4),
        ("va_guo_hall_thinning_u8", "h = VA_THIN_MAX_ROWS + 1"): _thinning_abi(ops, 1, 65535 * 32 + 1, 1),
        ("va_resize_u8", "dst_h = 65536"): _resize_abi(ops, np.uint8),
        ("va_resize_f32", "dst_h = 65536"): _resize_abi(ops, np.float32),
    }
    assert set(calls) == set(REFUSED)
    for (entry, case), call in calls.items():
        _refused(entry, case, call)
    # the largest target those limits admit computes
    src = np.arange(8, dtype=np.uint8).reshape(1, 2, 4)
    _equal(ops.resize(src, (1, 65535), "nearest"), oracle.resize_u8(src, (1, 65535), "nearest"), "65535 target rows")
