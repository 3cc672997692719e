"""GPU: the float paths on non-finite, subnormal and extreme values ("Special values").

Every image-valued float op runs on the benign random image of the other GPU tests with the value classes of
tests/special_values_checks.py written in -- NaN, the infinities, signed zeros, subnormals, FLT_MIN, +-FLT_MAX and a
pair of 3e38 whose sum overflows -- and every caller-owned state (va_bg_set_state, BackgroundModel(background=...),
running_mean(mean=...), welford(mean=, m2=)) holds their float64 / float32 counterparts.  Every comparison is
`same_floats` against the oracle or the project's restatement of the op: the same NaN mask and the same bits
everywhere else, no tolerance (image_statistics with a fractional prior keeps the tolerance of
tests/test_gpu_parity.py:551).  tests/test_special_values_host.py shows, without a GPU, that the references stay
inside defined C on exactly these inputs.

Not compared, because C leaves the conversion undefined: the uint8 difference image of a background model whose
state is NaN (those cases update the state alone), and normalize to uint8 outside [0, 256).

Left out on purpose: snakes and optical flow iterate with control flow whose behaviour on NaN the reference does not
define; peak detection has its infinities and signed zeros pinned by the reference fixture, and its NaN behaviour
follows scipy's unspecified comparison order.
"""
import importlib.util
import os

import numpy as np
import pytest

import special_values_checks as S
from special_values_checks import same_floats
from test_gpu_bg_mean_paths import FORMS, _update

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REFS = {}


def _ref(key, make):
    """a reference or an input, made once and left unchanged"""
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


def _generator(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---------------------------------------------------------------------------------------------- Gaussian
@pytest.mark.parametrize("hook", [0, 1, 3])
@pytest.mark.parametrize("case", range(len(S.GAUSS_SHAPES)))
def test_gaussian_f32(oracle, case, hook):
    """sigma 1 and 2 have compile-time radii, 3.3 a runtime radius; hook 1: runtime-radius columns, 3: rows too"""
    from video import _hip, ops
    shape, color = S.GAUSS_SHAPES[case]
    im = _ref(("gauss_in", case), lambda: S.gaussian_input(shape, color))
    _hip.check(_hip.lib().va_test_hook_gaussian_f32(hook))
    try:
        for sigma in S.GAUSS_SIGMAS:
            want = _ref(("gauss", case, sigma), lambda: oracle.gaussian_f32(im, sigma))
            same_floats(ops.gaussian_blur(im, sigma, color=color), want, (shape, sigma, hook))
    finally:
        _hip.check(_hip.lib().va_test_hook_gaussian_f32(0))


# --------------------------------------------------------------------------------------- float32 engine
@pytest.mark.parametrize("per_run", [1, 4])
def test_engine_float32_chain(oracle, per_run):
    """EMA + Gaussian in the fused kernels (the engine of test_gpu_hostile_memory.test_engine_float32_chain), specials
    in the frames and in a state set through set_background"""
    from video.engine import FrameEngine
    clip = _ref(("eng_in",), S.engine_clip)
    n, h, w, c = clip.shape
    eng = FrameEngine(size=(w, h), channels=c, dtype=np.float32, max_batch=4, background="ema", bg_rate=S.ENGINE_RATE,
                      sigma=S.ENGINE_SIGMA)
    try:
        for n_seen, state in _ref(("eng_cases",), S.engine_cases):
            def reference():
                d, bg = oracle.bg_ema_f32(clip, bg=state, n_seen=n_seen, rate=S.ENGINE_RATE)
                return oracle.gaussian_f32(d, S.ENGINE_SIGMA), bg
            blur, bg = _ref(("eng", n_seen), reference)
            eng.set_background(state, n_seen)
            got = np.concatenate([eng.run(clip[a:a + per_run], want=("filtered",))["filtered"]
                                  for a in range(0, n, per_run)])
            same_floats(got, blur, (per_run, n_seen, "filtered"))
            got_bg, seen = eng.get_background()
            assert seen == n_seen + n
            same_floats(got_bg, bg, (per_run, n_seen, "state"))
    finally:
        eng.close()


# ----------------------------------------------------------------------------------------- va_bg_update
def _model_run(mode, dtype, frames, state, n_seen, want_diff=True):
    """ops.BackgroundModel(background=state) at n_seen over `frames`: (difference images or None, new state)"""
    from video import ops
    m = ops.BackgroundModel(frames.shape[1:], mode, rate=S.EMA_RATE, dtype=dtype, background=state)
    try:
        m.n_seen = int(n_seen)
        return m.process(frames, want_diff), m.state
    finally:
        m._state.free()


def test_bg_update_ema_f32(oracle):
    for k, (fr, st, n_seen) in enumerate(_ref(("ema_f32_cases",), S.ema_f32_cases)):
        d, bg = _ref(("ema_f32", k), lambda: oracle.bg_ema_f32(fr, bg=st, n_seen=n_seen, rate=S.EMA_RATE))
        for want_diff in (True, False):
            got_d, got_bg = _model_run("ema", np.float32, fr, st, n_seen, want_diff)
            if want_diff:
                same_floats(got_d, d, (fr.shape, n_seen))
            same_floats(got_bg, bg, (fr.shape, n_seen, want_diff))


def test_bg_update_ema_u8(oracle):
    """float32 special states under uint8 frames; a NaN state (and an infinite one beyond its first frame) has no
    defined difference image: state only"""
    for k, (fr, st, n_seen, want_diff) in enumerate(_ref(("ema_u8_cases",), S.ema_u8_cases)):
        def reference():
            if want_diff:
                return oracle.bg_ema_u8(fr, bg=st, n_seen=n_seen, rate=S.EMA_RATE)
            return None, S.ema_u8_state_only(oracle, fr, st, n_seen)
        d, bg = _ref(("ema_u8", k), reference)
        got_d, got_bg = _model_run("ema", np.uint8, fr, st, n_seen, want_diff)
        where = (fr.shape, n_seen, want_diff)
        if want_diff:
            assert np.array_equal(got_d, d), where
        same_floats(got_bg, bg, where)


def test_bg_update_static_u8(oracle):
    for fr, st in _ref(("static_cases",), S.static_cases):
        got_d, got_bg = _model_run("static", np.uint8, fr, st, 0)
        assert np.array_equal(got_d, oracle.bg_static_u8(fr, st)), fr.shape
        same_floats(got_bg, st, fr.shape)


def _mean_reference(oracle, form, n_seen, n, want_diff):
    fr, st = S.mean_u8_case(FORMS[form][0], n_seen, n, want_diff)
    ref = _ref(("mean", FORMS[form][0], n_seen, n, want_diff),
               lambda: oracle.bg_mean_u8(fr, mean=st, n_seen=n_seen, want_diff=want_diff))
    return fr, st, ref


@pytest.mark.parametrize("form", sorted(FORMS))
def test_bg_update_mean_u8(oracle, form):
    """the running mean from every special float64 state, under frames that hold 0, 255 and both in turn: the
    division-free kernels at 16 and 8 pixels per thread and the plain-division kernel (scalar, the control).  Every
    special value has a thread of its own (special_values_checks.special_state, group = 16): the values inside the
    kernels' domain -- +-0.0 and its edges -- go through the division-free arithmetic, under runs of zero pixels too,
    and every value outside it sends its thread through plain divisions alone (the host test asserts that layout)"""
    late = FORMS[form][1]
    for n_seen in S.MEAN_N_SEEN:
        for n in S.MEAN_N:
            for want_diff in (True, False):
                fr, st, (ref_d, ref_st) = _mean_reference(oracle, form, n_seen, n, want_diff)
                got_d, got_st = _update(fr, st, n_seen, want_diff, late)
                where = (form, n_seen, n, want_diff)
                if want_diff:
                    assert np.array_equal(got_d, ref_d), where
                same_floats(got_st, ref_st, where)


@pytest.mark.parametrize("form", ["narrow", "scalar", "wide"])
def test_mean_u8_through_engine_model_and_running_mean(oracle, form):
    """the same states through FrameEngine.set_background (which chooses the bounded or the saturating kernels from
    the state it is given), ops.BackgroundModel and ops.running_mean(mean=...)"""
    from video import ops
    from video.engine import FrameEngine
    n = S.ENGINE_MEAN_N
    shape = S.form_shape(FORMS[form][0], len(S.MEAN_STATES))
    eng = FrameEngine(size=(shape[1], shape[0]), max_batch=n, background="mean")
    try:
        for n_seen in S.ENGINE_MEAN_N_SEEN:
            fr, st, (ref_d, ref_st) = _mean_reference(oracle, form, n_seen, n, True)
            assert fr.shape[1:] == shape
            eng.set_background(st, n_seen)
            got_d = eng.run(fr, want=("filtered",))["filtered"]
            got_st, seen = eng.get_background()
            assert seen == n_seen + n and np.array_equal(got_d, ref_d), (form, n_seen)
            same_floats(got_st, ref_st, (form, n_seen, "engine"))
            got_d, got_st = _model_run("mean", np.uint8, fr, st, n_seen)
            assert np.array_equal(got_d, ref_d), (form, n_seen)
            same_floats(got_st, ref_st, (form, n_seen, "model"))
            fr, st, (_, ref_st) = _mean_reference(oracle, form, n_seen, n, False)       # (with the NaN state)
            eng.set_background(st, n_seen)
            eng.run(fr, want=("filtered",))                      # (its difference under the NaN state is not compared)
            same_floats(eng.get_background()[0], ref_st, (form, n_seen, "engine, all states"))
            same_floats(ops.running_mean(fr, st, n_seen), _ref(("mean_any_u8", form, n_seen),
                                                               lambda: oracle.mean_any(fr, st, n_seen)), (form, n_seen))
            same_floats(oracle.mean_any(fr, st, n_seen), ref_st, (form, n_seen, "oracle"))
            # states inside [0, 255]: the pipeline vouches for the range and runs the kernels without the saturation
            fr, st = S.bounded_mean_case(FORMS[form][0], n)
            assert fr.shape[1:] == shape and st.min() >= 0 and st.max() <= 255
            ref_d, ref_st = oracle.bg_mean_u8(fr, mean=st, n_seen=n_seen)
            eng.set_background(st, n_seen)
            got_d = eng.run(fr, want=("filtered",))["filtered"]
            assert np.array_equal(got_d, ref_d), (form, n_seen, "bounded")
            same_floats(eng.get_background()[0], ref_st, (form, n_seen, "bounded"))
    finally:
        eng.close()


# ------------------------------------------------------------------------------ running_mean and welford
@pytest.mark.parametrize("case", range(7))
def test_running_mean_and_welford(oracle, case):
    """float32 / float64 frames with the specials and int16 frames at their extremes, from zero states and from
    special mean / m2 states; float32 frames also where float32(n + 1) rounds.  float64 frames against NumPy's
    restatement, which the host test ties to the C oracle"""
    from video import ops
    cases = _ref(("temporal_cases",), S.temporal_cases)
    assert len(cases) == 7
    fr, mean, m2, n_seen = cases[case]
    m0 = np.zeros(fr.shape[1:]) if mean is None else mean
    q0 = np.zeros(fr.shape[1:]) if m2 is None else m2
    if fr.dtype == np.float64:
        want_mean, want_w = S.mean_numpy(fr, m0, n_seen), S.welford_numpy(fr, m0, q0, n_seen)
    else:
        want_mean, want_w = oracle.mean_any(fr, mean, n_seen), oracle.welford_any(fr, mean, m2, n_seen)
    where = (fr.dtype, n_seen, mean is None)
    same_floats(ops.running_mean(fr, mean, n_seen), want_mean, where)
    got = ops.welford(fr, mean, m2, n_seen)
    same_floats(got[0], want_w[0], where)
    same_floats(got[1], want_w[1], where)
    # split over two calls: the state that goes round is the special one the first call left
    half = ops.welford(fr[:2], mean, m2, n_seen)
    got = ops.welford(fr[2:], half[0], half[1], n_seen + 2)
    same_floats(got[0], want_w[0], where)
    same_floats(got[1], want_w[1], where)


def test_welford_u8_special_states(oracle):
    from video import ops
    fr, st = S.mean_u8_case(FORMS["wide"][0], 5, 9, False)
    m2 = st[::-1].copy()
    want = oracle.welford_u8(fr, st, m2, 5)
    got = ops.welford(fr, st, m2, 5)
    same_floats(got[0], want[0])
    same_floats(got[1], want[1])


# ------------------------------------------------------------------------------------------- normalize
@pytest.mark.parametrize("target", [np.float32, np.float64])
def test_normalize_float_targets(target):
    """float32 frames stay float32 until the final astype; the bounds meet NaN, both infinities and subnormals"""
    from video import ops
    f = _ref(("norm_in",), lambda: S.special_frames((2, 9, 13), 8))
    assert np.isnan(f).any() and np.isinf(f).any()
    for fmin, fmax, alpha, tmin in S.NORMALIZE_BOUNDS:
        want = S.normalize_numpy(f, fmin, fmax, alpha, tmin, target)
        same_floats(ops.normalize_any(f, fmin, fmax, alpha, tmin, target), want, (target, fmin, fmax))


def test_normalize_uint8_target_in_range():
    from video import ops
    f = S.normalize_u8_input()
    bounds = ((0.0, 1.0, 255.0, 0.0), (S.FLT_SUB_MIN, 0.5, 510.0, 0.75), (-0.0, 1.0, 200.0, 55.0))
    for fmin, fmax, alpha, tmin in bounds:
        want = S.normalize_numpy(f, fmin, fmax, alpha, tmin, np.uint8)
        got = ops.normalize_any(f, fmin, fmax, alpha, tmin, np.uint8)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (fmin, fmax)


# ---------------------------------------------------------------------------------------------- resize
@pytest.mark.parametrize("mode", S.RESIZE_MODES)
def test_resize_f32(oracle, mode):
    from video import ops
    for name, (im, color, sizes) in _ref(("resize_in",), S.resize_inputs).items():
        for size in sizes:
            want = _ref(("resize", name, size, mode),
                        lambda: oracle.resize_f32(im, size, mode, layout="hwc" if color else None))
            same_floats(ops.resize(im, size, mode, color=color), want, (name, size, mode))


# ---------------------------------------------------------------------------- Sobel and ragged gradients
def _bits64(a):
    return np.ascontiguousarray(a, np.float64)


def test_sobel5_f64():
    """the centre tap's 0.0 * m turns an infinite centre pixel into NaN"""
    from video import ops
    AG = _generator("make_golden_active_contour")
    x = _ref(("sobel_in",), lambda: S.special_frames((2, 33, 70), 12))
    with np.errstate(all="ignore"):
        want = AG.sobel5(x)
    ys, xs = np.nonzero(np.isinf(x[1]))
    assert len(ys) and all(np.isnan(want[0][1, y, x_]) for y, x_ in zip(ys, xs))
    assert np.isfinite(want[0][0]).mean() > 0.5
    gx, gy = ops.sobel5_f64(x)
    same_floats(_bits64(gx), _bits64(want[0]), "fx")
    same_floats(_bits64(gy), _bits64(want[1]), "fy")


@pytest.mark.parametrize("sigma", [0.0, 1.0])
def test_potential_gradients_ragged(sigma):
    from video import ops
    AG = _generator("make_golden_active_contour")
    items = _ref(("grad_in",), S.gradient_items)
    with np.errstate(all="ignore"):
        want = [AG.gradients(p, sigma) for p in items]
    total = sum(p.size for p in items)
    fx, fy, shapes, offsets = ops.potential_gradients_ragged(items, sigma)
    try:
        flats = [b.download((total,), np.float64) for b in (fx, fy)]
    finally:
        fx.free()
        fy.free()
    for k, ((h, w), o) in enumerate(zip(shapes.tolist(), offsets.tolist())):
        for flat, plane in zip(flats, want[k]):
            same_floats(flat[o:o + h * w].reshape(h, w), _bits64(plane), (sigma, k))


# ------------------------------------------------------------------------------------ image statistics
def test_image_statistics_f32(oracle):
    """-0.5, -0.0 and subnormals truncate to 0; 2^31 (what float32 makes of 2^31 + 0.5), +-(2^31 + 256) and 2^40 are
    past int32 and inside int64, -2^31 is the last value inside int32.  Integer priors: bit for bit; a fractional
    prior with the tolerances of tests/test_gpu_parity.py:551"""
    from video import ops
    img = S.statistics_input()
    assert (img == 2.0 ** 31).sum() == 3 and (img == -2.0 ** 31).sum() == 3 and (abs(img) > 2.0 ** 31).sum() == 9
    for kernel, ksize, prior, excl in (("box", 3, 10, False), ("ellipse", 4, 0, True), ("box", 1, 2.5, False)):
        gm, gv = ops.image_statistics(img, kernel, ksize, prior, excl)
        rm, rv = oracle.image_statistics(img, kernel, ksize, prior, excl)
        if float(prior).is_integer():
            same_floats(gm, rm, (kernel, ksize))
            same_floats(gv, rv, (kernel, ksize))
        else:
            assert np.allclose(gm, rm, rtol=1e-12, atol=1e-12) and np.allclose(gv, rv, rtol=1e-10, atol=1e-9)
