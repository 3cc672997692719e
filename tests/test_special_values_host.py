"""No GPU: the references of tests/test_gpu_special_values.py can be trusted on non-finite, subnormal and extreme
inputs ("Special values").

  * oracle/va_oracle.c, linked into a stand-alone program with -fsanitize=undefined,float-cast-overflow, stays inside
    defined C on every input whose output the GPU test compares -- and leaves it on the inputs the GPU test takes out;
  * the inputs do their work: the non-finite values do not flood the references, every value class changes them, and a
    resize case has a zero-weight tap next to a non-finite pixel;
  * NumPy's restatement of measure_mean / measure_mean_std, the reference for float64 frames, agrees with the C oracle
    on float32 and int16 frames;
  * the running mean's division-free quotient, three lines of C, differs from the plain division exactly where
    va_point.hip says it does, and nowhere in the domain the kernel keeps it to.
"""
import numpy as np
import pytest

import special_values_checks as S

MEAN_BASE_SHAPES = [(16, 24), (8, 9), (5, 7)]          # the shapes of test_gpu_bg_mean_paths.FORMS


def test_forms_are_those_of_the_running_mean_test():
    import test_gpu_bg_mean_paths as P
    assert sorted(set(shape for shape, _ in P.FORMS.values())) == sorted(MEAN_BASE_SHAPES)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("special_values")
    return S.compile_driver(d), d


def _outputs(out, wants):
    pos = 0
    for w in wants:
        yield np.frombuffer(out[pos:pos + w.nbytes], w.dtype).reshape(w.shape), w
        pos += w.nbytes
    assert pos == len(out)


# ------------------------------------------------------------------------------------- the sanitized oracle
def test_oracle_stays_inside_defined_c(oracle, driver):
    """every oracle call behind the GPU test, in one run of the program: exit 0, and the outputs of the sanitized -O1
    build are those of the library the tests load"""
    exe, d = driver
    calls = S.oracle_calls(oracle, MEAN_BASE_SHAPES)
    assert len(calls) > 200
    rc, err, out = S.run_driver(exe, d, [c[1] for c in calls])
    assert rc == 0, err[-3000:]
    names = [name for name, _, wants in calls for _ in wants]
    for name, (g, w) in zip(names, _outputs(out, [w for _, _, wants in calls for w in wants])):
        if w.dtype.kind == "f":
            S.same_floats(g, w, name)
        else:
            assert np.array_equal(g, w), name


@pytest.mark.parametrize("op", ["bg_mean_u8", "bg_ema_u8", "bg_static_u8"])
def test_what_the_gpu_test_leaves_out_is_undefined(driver, op):
    """a NaN state under a uint8 difference image: the program stops at the conversion.  So the check above can
    fail, and the state-only runs of these cases are not a convenience"""
    exe, d = driver
    fr = np.full((1, 8), 7, np.uint8)
    st = np.full(8, np.nan, np.float32 if op == "bg_ema_u8" else np.float64)
    ints = (1, 8) if op == "bg_static_u8" else (1, 8, 3, 1)
    rc, err, _ = S.run_driver(exe, d, [S.record(op, ints, (S.EMA_RATE,), (fr, st))], name="nan_" + op)
    assert rc != 0 and "runtime error" in err and "outside the range" in err, (rc, err[-500:])
    if op != "bg_static_u8":
        rc, err, _ = S.run_driver(exe, d, [S.record(op, (1, 8, 3, 0), (S.EMA_RATE,), (fr, st))], name="nan_state_" + op)
        assert rc == 0, err[-500:]


# ----------------------------------------------------------------------------------------------- the inputs
def _finite_share(a):
    return np.isfinite(a).mean()


def test_nonfinite_values_do_not_flood(oracle):
    """at least a quarter of every Gaussian / resize / EMA reference output is finite"""
    for name, _, wants in S.oracle_calls(oracle, MEAN_BASE_SHAPES[:1]):
        if name[0] in ("gaussian", "resize", "engine ema", "engine gaussian", "ema f32"):
            for w in wants:
                assert _finite_share(w) >= 0.25, (name, _finite_share(w))
                assert not np.isfinite(w).all() or name[0] == "resize", name        # ... and some of it is not


@pytest.mark.parametrize("cls", sorted(S.F32_CLASSES))
def test_every_class_changes_the_references(oracle, cls):
    """the class alone, written into the benign image, changes the output of the Gaussian, of the resize and of the
    EMA"""
    for shape, color in S.GAUSS_SHAPES:
        plain, only = S.gaussian_input(shape, color, "none"), S.gaussian_input(shape, color, cls)
        assert S.differs(only, plain), (cls, shape)
        for sigma in S.GAUSS_SIGMAS:
            assert S.differs(oracle.gaussian_f32(only, sigma), oracle.gaussian_f32(plain, sigma)), (cls, shape, sigma)
    plain, only = S.resize_stack("none"), S.resize_stack(cls)
    for size in ((60, 45), (7, 5), (120, 90)):
        for mode in S.RESIZE_MODES:
            if size == (7, 5) and mode != "area":
                continue                        # (35 samples of a few taps each: most of a class's pixels are not read)
            assert S.differs(oracle.resize_f32(only, size, mode), oracle.resize_f32(plain, size, mode)), (cls, size,
                                                                                                          mode)
    plain, only = S.special_frames((4, 9, 13), 63, only="none"), S.special_frames((4, 9, 13), 63, only=cls)
    if cls != "pair":                           # (the plane is too small for the pair's runs: plant())
        for a, b in zip(oracle.bg_ema_f32(only, n_seen=3, rate=S.EMA_RATE),
                        oracle.bg_ema_f32(plain, n_seen=3, rate=S.EMA_RATE)):
            assert S.differs(a, b), cls


def test_the_pair_overflows_in_the_column_pass_alone(oracle):
    """a + b of the oracle's symmetric column pass (va_oracle.c, vao_gaussian_f32) is infinite between the two runs of
    3e38, where the same taps applied one by one stay finite"""
    for sigma in S.GAUSS_SIGMAS:
        im = S.benign((1, 37, 53), 1)
        S.plant(im[0], ["pair"])
        out = oracle.gaussian_f32(im, sigma)[0]
        taps = oracle.gauss_taps_f32(sigma).astype(np.float64)
        r = len(taps) // 2
        pad = np.pad(im[0].astype(np.float64), r, mode="reflect")
        k = range(len(taps))
        one_by_one = sum(taps[i] * taps[j] * pad[i:i + 37, j:j + 53] for i in k for j in k)
        assert np.isinf(out[37 // 2, 5]) and np.isfinite(one_by_one).all() and abs(one_by_one).max() < S.FLT_MAX, sigma
        assert np.isfinite(out[1, 53 // 2]), sigma              # the pair about a column: the row pass adds tap by tap


def test_a_zero_weight_tap_meets_a_nonfinite_pixel(oracle):
    """linear and cubic at three times the size land on integer source coordinates: output (3y + 1, 3x + 1) is source
    pixel (y, x) with weight 1 and its neighbours with weight 0, and 0 * Inf is NaN"""
    im, _, sizes = S.resize_inputs()["stack"]
    assert (120, 90) in sizes
    for mode in ("linear", "cubic"):
        out = oracle.resize_f32(im, (120, 90), mode)
        centre = out[:, 1::3, 1::3]
        assert centre.shape == im.shape
        hit = np.isfinite(im) & np.isnan(centre)
        assert hit.sum() >= 3, (mode, int(hit.sum()))
        clean = np.isfinite(im) & np.isfinite(centre)
        assert np.array_equal(centre[clean], im[clean]) or mode == "cubic"


# --------------------------------------------------------------------- NumPy's restatement and the C oracle
def test_numpy_restatement_agrees_with_the_oracle(oracle):
    """float64 frames have no entry in va_oracle.c; their reference is the arithmetic of oracle.measure_mean_numpy and
    oracle.measure_mean_std_numpy, which on float32 and int16 frames is the C oracle's, special values included"""
    seen = set()
    for fr, mean, m2, n_seen in S.temporal_cases():
        if fr.dtype == np.float64:
            continue
        seen.add((fr.dtype.name, mean is None, n_seen))
        m0 = np.zeros(fr.shape[1:]) if mean is None else mean
        q0 = np.zeros(fr.shape[1:]) if m2 is None else m2
        where = (fr.dtype, n_seen)
        S.same_floats(S.mean_numpy(fr, m0, n_seen), oracle.mean_any(fr, mean, n_seen), where)
        wm, wq = S.welford_numpy(fr, m0, q0, n_seen)
        om, oq = oracle.welford_any(fr, mean, m2, n_seen)
        S.same_floats(wm, om, where)
        S.same_floats(wq, oq, where)
        if mean is None and n_seen == 0:
            with np.errstate(all="ignore"):
                S.same_floats(oracle.measure_mean_numpy(fr), oracle.mean_any(fr), where)
    assert len(seen) == 5 and ("float32", True, S.ROUNDING_N_SEEN) in seen
    fr = S.temporal_frames(np.float32)
    assert not np.isfinite(fr).all() and np.isfinite(fr).mean() > 0.5
    assert int(np.float32(S.ROUNDING_N_SEEN + 2)) != S.ROUNDING_N_SEEN + 2     # the divisor does round


# ------------------------------------------------------------------------- the division-free quotient's model
def _model(driver, x, d):
    exe, directory = driver
    x, d = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(d, np.float64)
    rc, err, out = S.run_driver(exe, directory, [S.record("div_model", (x.size,), (), (x, d))], name="div_model")
    assert rc == 0, err[-500:]
    both = np.frombuffer(out, np.float64).reshape(2, x.size)
    assert np.array_equal(both[1], x / d, equal_nan=True)
    return both[0], both[1]


def test_division_free_quotient_outside_its_domain(driver):
    """the two divergences that va_point.hip's comment names: an infinite or overflowed numerator gives NaN where the
    division gives Inf, and subnormal numerators lose half-way cases"""
    with np.errstate(all="ignore"):
        inf = float("inf")
        x = [inf, -inf, np.float64(1e308) * 2, np.float64(S.DBL_MAX) * 5]      # the states Inf, 1e308, DBL_MAX times n
        model, plain = _model(driver, x, [6.0, 6.0, 3.0, 6.0])
        assert np.isnan(model).all() and np.array_equal(plain, [inf, -inf, inf, inf])
        sub = 2.0 ** -1074
        model, plain = _model(driver, [9 * 5 * sub], [6.0])          # the state 9 * 2^-1074 at n_seen = 5
        assert plain[0] == 8 * sub and model[0] == 7 * sub
        k, n = np.meshgrid(np.arange(1, 4001), np.arange(0, 301))
        x = (k * sub) * n
        model, plain = _model(driver, x.ravel(), (n + 1.0).ravel())
        assert x.size == 1204000 and int((model != plain).sum()) == 3598
        model, plain = _model(driver, [-0.0], [6.0])
        assert np.signbit(plain[0]) and not np.signbit(model[0]) and model[0] == 0.0


def test_division_free_quotient_inside_its_domain(driver):
    """bit-identical to the division for x = 0 and 2^-960 <= |x| <= 2^1020 (the domain va_point.hip states), at both
    edges and across it, for the divisors a frame count gives: all of 1 .. 4096 and random integers below 2^53"""
    rng = np.random.default_rng(2)
    count = 400000
    d = np.concatenate([np.arange(1, 4097), rng.integers(1, 2 ** 53, count - 4096)]).astype(np.float64)
    mant = 1.0 + rng.random(count)
    sign = np.where(rng.random(count) < 0.5, -1.0, 1.0)
    for name, expo in (("low edge", rng.integers(-960, -940, count)), ("high edge", rng.integers(1000, 1020, count)),
                       ("across", rng.integers(-960, 1020, count))):
        x = sign * np.ldexp(mant, expo)
        model, plain = _model(driver, x, d)
        assert np.isfinite(plain).all() and np.array_equal(model, plain), name
    x = np.concatenate([np.ldexp(1.0, [-960, 1020]), [0.0], rng.integers(0, 256, 1000).astype(np.float64)])
    model, plain = _model(driver, x, d[:x.size])
    assert np.array_equal(model, plain) and not np.signbit(model[2])


def test_every_special_state_decides_its_thread_alone():
    """the layout behind test_gpu_special_values.test_bg_update_mean_u8: in the kernels that own 16 and 8 pixels per
    thread, the thread of a special value holds no other one, so a value inside the division-free domain (+-0.0, the
    last values inside its edges) stays on the fast path, under zero pixels too, and each value outside it (NaN,
    +-Inf, every subnormal, DBL_MIN, 2^-1000, +-1e300, 1e308, DBL_MAX, the first values outside the edges) is the one
    value that takes its thread off it: a guard without either of its bounds would be noticed"""
    L = len(S.MEAN_STATES)
    inside = S.in_fast_domain(S.MEAN_STATES)
    assert [bool(b) for b in inside] == [v == 0 for v in S.F64_STATES] + [True, False, True, False, True, False]
    cases = [S.mean_u8_case(base, n_seen, n, want_diff)[::-1] + (S.mean_states(n_seen, want_diff),)
             for base in MEAN_BASE_SHAPES[:2] for n_seen in (0, 5) for n in (1, 40) for want_diff in (True, False)]
    cases += [(st, fr, [v for v in S.MEAN_STATES if 0 <= v <= 255])
              for base in MEAN_BASE_SHAPES[:2] for fr, st in [S.bounded_mean_case(base, 9)]]
    assert len(cases[1][2]) == L
    for st, fr, values in cases:
        assert st.shape == fr.shape[1:] and st.size % 8 == 0
        flat, pixels = st.reshape(-1), fr.reshape(len(fr), -1)
        for v in (8, 16):
            if st.size % v:
                continue
            fast = S.fast_threads(st, v)
            special = np.zeros(st.size, bool)
            for c, slots in enumerate(S.special_slots(len(values), 3, S.MEAN_GROUP)):
                special[slots] = True
                for value, at in zip(values, slots):
                    assert flat[at] == value or (np.isnan(value) and np.isnan(flat[at]))
                    assert bool(fast[at // v]) == bool(S.in_fast_domain(value)), (v, value, c)
                    others = np.delete(flat[at // v * v:(at // v + 1) * v], at % v)
                    assert S.in_fast_domain(others).all() and (others > 1e-9).all(), (v, value, c)
                    want = {0: [0], 1: [255], 2: [0, 255][:len(fr)]}[c]
                    assert sorted(set(pixels[:, at].tolist())) == want, (v, value, c)
            assert S.in_fast_domain(flat[~special]).all()
            assert int((~fast).sum()) == 3 * int((~S.in_fast_domain(values)).sum())
    # the launch-long half of the argument is run on the card: 2^-900 under 40 zero pixels at the largest n_seen
    assert 2.0 ** -900 in S.mean_states(S.MEAN_N_SEEN[-1], True) and max(S.MEAN_N) == 40


def test_the_kernels_bounds_are_those_of_the_tests():
    """kFastMeanMin / kFastMeanMax of va_point.hip are the bounds the layout above is built on"""
    import os
    with open(os.path.join(S.ROOT, "video-analysis_amd", "csrc", "va_point.hip")) as f:
        text = f.read()
    assert "constexpr double kFastMeanMin = %s, kFastMeanMax = %s;" % (
        float.hex(S.FAST_MEAN_MIN).replace("0x1.0000000000000p", "0x1p"),
        float.hex(S.FAST_MEAN_MAX).replace("0x1.0000000000000p", "0x1p").replace("p+", "p")) in text
