"""CPU: the pinned definition of the equidistant resampling ("Equidistant curves").  The scalar
restatement of tests/curves_checks.py equals curves.make_curve_equidistant on the fixture curves and on seeded
random ones; va_curves_math.h, compiled with the host compiler, equals math.hypot, the restatement and the NumPy
function; the entry point is declared and bound; ops.curves_equidistant checks its arguments and routes what the
device does not take.  Comparisons are on the bit patterns."""
import math
import os

import numpy as np
import pytest

import curves_checks as K
from curves_checks import bits_equal

ROOT = K.ROOT
MODES = (dict(), dict(count=11), dict(spacing=2.5))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = K.compile_shim(tmp_path_factory.mktemp("curves_shim"))
    if lib is None:
        pytest.skip("no host C++ compiler")
    return lib


def _polygon_centerlines():
    z = np.load(os.path.join(ROOT, "tests", "golden", "polygon_v1.npz"))
    return {k: z[k] for k in z.files if k.startswith(("est/", "opt/")) and z[k].ndim == 2 and z[k].shape[1] == 2
            and len(z[k]) >= 2}


# ------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("mode", range(len(MODES)))
def test_restatement_equals_the_function_on_the_fixture_curves(mode):
    from video.analysis import curves
    kw = MODES[mode]
    inputs, z = K.fixture_curves()
    assert sorted(inputs) == ["ellipse", "int", "wiggle"]
    key = "equidistant_spacing" if "spacing" in kw else "equidistant_count" if "count" in kw else "equidistant"
    for name, pts in inputs.items():
        want = np.asarray(curves.make_curve_equidistant(pts, **kw))
        assert bits_equal(K.equidistant(pts, **kw), want), name
        assert bits_equal(want, z["curves/%s/%s" % (name, key)]), name     # (what the reference's own code wrote)


def test_restatement_equals_the_function_on_the_stored_centerlines():
    from video.analysis import curves
    lines = _polygon_centerlines()
    assert len(lines) >= 20
    for name, pts in lines.items():
        for kw in MODES + (dict(spacing=20), dict(spacing=5)):
            assert bits_equal(K.equidistant(pts, **kw), np.asarray(curves.make_curve_equidistant(pts, **kw))), (name, kw)


def test_restatement_equals_the_function_on_random_curves():
    from video import ops
    from video.analysis import curves
    if not ops.host_norm_is_pinned():
        pytest.skip("this host's np.linalg.norm is not sqrt(fma(dy, dy, dx * dx)): the walk is pinned to that form")
    sizes = set()
    for c in K.mixed_curves(11, 45, 2, 60):
        for sp in (0.7, 2.5, 10, 20):
            want = np.asarray(curves.make_curve_equidistant(c, spacing=sp))
            assert bits_equal(K.equidistant(c, spacing=sp), want)
            L = curves.curve_length(c)
            if L >= sp:
                sizes.add(len(want) - int(np.round(L / sp)))
        for ct in (None, 1, 2, 4 * len(c)):
            assert bits_equal(K.equidistant(c, count=ct), curves.make_curve_equidistant(c, count=ct))
    assert {1, 2} <= sizes          # both result sizes occur: rint(L / spacing) + 1 and + 2


def test_norm_guard_reads_the_fused_form():
    from video import ops
    for x, y, fused, plain in ops._NORM_PROBES:
        x, y, fused, plain = (float.fromhex(v) for v in (x, y, fused, plain))
        assert K.norm2(x, y) == fused and math.sqrt(x * x + y * y) == plain and fused != plain
    assert ops.host_norm_is_pinned() in (True, False)


# ------------------------------------------------------------------------------------------- the math header
def _hypot_pairs():
    """1.2 million pairs: floats over sixteen decades, integer lattices, equal and zero components, and pairs
    beyond 2^500 and below 2^-500, which the header scales"""
    rng = np.random.default_rng(5)
    xs, ys = [], []

    def floats(n):
        a = rng.normal(size=(n, 2)) * 10 ** rng.uniform(-8, 8, (n, 2))
        return a[:, 0].copy(), a[:, 1].copy()
    x, y = floats(600000)
    xs.append(x), ys.append(y)
    lattice = rng.integers(-3000, 3000, (300000, 2)).astype(np.float64)
    xs.append(lattice[:, 0].copy()), ys.append(lattice[:, 1].copy())
    x, _ = floats(50000)
    xs.append(x), ys.append(x.copy())
    x, _ = floats(50000)
    xs.append(x), ys.append(np.zeros_like(x))
    for lo, hi in ((501, 1020), (-1000, -501)):
        v = np.ldexp(rng.uniform(0.5, 1, (100000, 2)), rng.integers(lo, hi, (100000, 1)) + rng.integers(-3, 1, (100000, 2)))
        xs.append(v[:, 0].copy()), ys.append(v[:, 1].copy())
    return np.concatenate(xs), np.concatenate(ys)


def test_header_hypot_equals_math_hypot(shim):
    x, y = _hypot_pairs()
    assert len(x) >= 10 ** 6
    got = np.empty_like(x)
    shim.cs_hypot(x.ctypes.data, y.ctypes.data, got.ctypes.data, len(x))
    want = np.array([math.hypot(a, b) for a, b in zip(x.tolist(), y.tolist())])
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert len(bad) == 0, (len(bad), x[bad[:3]], y[bad[:3]])
    # ... and both are the correctly rounded root, on a sample
    for i in np.random.default_rng(6).choice(len(x), 2000, replace=False):
        assert K.hypot(float(x[i]), float(y[i])) == got[i], (x[i], y[i])


def test_header_norm_is_the_fused_form(shim):
    rng = np.random.default_rng(8)
    x, y = rng.normal(0, 5, 3000), rng.normal(0, 5, 3000)
    got = np.empty_like(x)
    shim.cs_norm2(x.ctypes.data, y.ctypes.data, got.ctypes.data, len(x))
    assert all(K.norm2(float(a), float(b)) == g for a, b, g in zip(x, y, got))
    assert np.count_nonzero(got != np.sqrt(x * x + y * y)) > 50       # (the plain form is another function)


def test_header_walk_and_interp_equal_the_restatement(shim):
    from video.analysis import curves
    inputs, _ = K.fixture_curves()
    cases = list(inputs.values()) + K.mixed_curves(12, 30, 2, 50)
    cases += [np.array([[0., 0.], [100., 0.]]), np.array([[1., 1.], [1., 1.], [4., 5.]]), np.full((5, 2), 3.25)]
    for c in cases:
        for sp in (0.7, 2.5, 20):
            got, length = K.shim_equidistant(shim, c, spacing=sp)
            assert bits_equal(got, K.equidistant(c, spacing=sp))
            assert length == curves.curve_length(got)
        for ct in (None, 1, 2, 11, 4 * len(c)):
            got, length = K.shim_equidistant(shim, c, count=ct)
            assert bits_equal(got, K.equidistant(c, count=ct))
            assert length == curves.curve_length(got)
    c = cases[0]
    got, length = K.shim_equidistant(shim, c, spacing=2.5, offset=(-7.0, 3.5))
    assert bits_equal(got, K.equidistant(c, spacing=2.5, offset=(-7.0, 3.5))) and length == curves.curve_length(got)
    assert bits_equal(got, curves.translate_points(np.asarray(curves.make_curve_equidistant(c, spacing=2.5)), -7.0, 3.5))
    assert shim.cs_length_f32(np.ascontiguousarray(c, np.float64).ctypes.data, len(c)) == curves.curve_length(c)
    assert shim.cs_spacing_count(np.ascontiguousarray(c, np.float64).ctypes.data, len(c), 0.01, 10) == -1   # the bound


# ------------------------------------------------------------------------------------------- the layers
def test_entry_point_is_declared_and_bound():
    from video import _hip
    text = open(os.path.join(ROOT, "include", "videoanalysis_hip.h")).read()
    assert "int va_curves_equidistant(" in text and "curves.py:103-148" in text
    assert len(_hip.SIGNATURES["va_curves_equidistant"][1]) == 16
    lib = _hip.load_library()
    assert hasattr(lib, "va_curves_equidistant")
    # argument checks run before anything touches a device
    assert lib.va_curves_equidistant(None, None, -1, 1, None, None, None, None, None, None, None, None, None, 0, None,
                                     None) == -22
    assert lib.va_curves_equidistant(None, None, 0, 1, None, None, None, None, None, None, None, None, None, 0, None,
                                     None) == -22 and b"NULL" in lib.va_last_error()
    assert lib.va_curves_equidistant(None, None, 0, 0, None, None, None, None, None, None, None, None, None, 0, None,
                                     None) == 0


def test_argument_checks_and_host_routing():
    from video import ops
    from video.analysis import curves
    line = np.array([[0., 0.], [3., 4.], [6., 8.]])
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops.curves_equidistant([line], spacing=bad)
        with pytest.raises(ValueError):
            curves.make_curves_equidistant([line], spacing=bad)
    with pytest.raises(ValueError):
        ops.curves_equidistant([line, line], count=[3])
    with pytest.raises(ValueError):
        ops.curves_equidistant([line], offsets=[(0, 0), (1, 1)])
    assert ops.curves_equidistant([]) == [] and curves.make_curves_equidistant([]) == []
    # what the device does not take goes through the host function: no GPU is touched
    one = np.array([[2., 3.]])
    nan = np.array([[0., 0.], [np.nan, 1.], [2., 2.]])
    huge = np.array([[0., 0.], [1e200, 1.]])
    got, lengths = ops.curves_equidistant([one, nan, huge], spacing=[5, None, None], count=[None, 4, 3],
                                          offsets=[(1, 2)] * 3, ret_lengths=True)
    assert bits_equal(got[0], one + [1, 2]) and lengths[0] == 0
    assert bits_equal(got[1], curves.translate_points(curves.make_curve_equidistant(nan, count=4), 1, 2))
    assert bits_equal(got[2], curves.translate_points(curves.make_curve_equidistant(huge, count=3), 1, 2))
    assert bits_equal([lengths[2]], [curves.curve_length(got[2])])          # (NaN: the float32 casts overflow)
    got = ops.curves_equidistant([line], count=0)
    assert got[0].shape == (0, 2)
    # below the threshold the batched callers stay on the host
    assert ops.CURVES_DEVICE_MIN_BATCH >= 2
    res, lengths = curves.resample_many([line], spacing=2.5, offsets=[(-1, 1)])
    assert bits_equal(res[0], curves.translate_points(np.asarray(curves.make_curve_equidistant(line, spacing=2.5)), -1, 1))
    assert lengths[0] == curves.curve_length(res[0])


def test_find_contours_raises_in_the_order_of_the_curves():
    """the batched resampling does not let a later curve's exception overtake an earlier curve's check"""
    from video import ops
    from video.analysis.active_contour import ActiveContour
    ac = ActiveContour()
    ac._grad = (None, None, (1, 8, 8))                   # (no device: every case below raises before a launch)
    try:
        nan = np.array([[0., 0.], [np.nan, 1.], [2., 2.], [3., 1.]])
        empty = np.zeros((0, 2))
        m = max(ops.CURVES_DEVICE_MIN_BATCH, 4)
        with pytest.raises(ValueError, match="curve 0 has non-finite points"):
            ac.find_contours([nan, empty] * m)
        with pytest.raises(ValueError) as err:
            ac.find_contours([empty, nan] * m)
        assert "non-finite" not in str(err.value)         # the empty curve's own error, as the loop gave it
        with pytest.raises(IndexError):
            ac.find_contours([nan[:1], empty], frames=[3, 0])
    finally:
        ac._grad = None
