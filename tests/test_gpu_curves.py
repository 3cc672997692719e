"""GPU: the batched equidistant resampling (va_curves_equidistant, ops.curves_equidistant,
curves.make_curves_equidistant) and its two callers, bit for bit against the per-curve function
curves.make_curve_equidistant ("Equidistant curves").  Where this host's np.linalg.norm is not the
form the walk is pinned to, the reference is the scalar restatement of tests/curves_checks.py instead.
Comparisons are on the bit patterns, so signed zeros count."""
import importlib.util
import os

import numpy as np
import pytest

import curves_checks as K
from curves_checks import bits_equal

pytestmark = pytest.mark.gpu

ROOT = K.ROOT


@pytest.fixture(scope="module")
def gpu():
    from video import _hip
    return _hip.lib()


def _want(curve, spacing=None, count=None, offset=None):
    """the per-curve result, translated"""
    from video import ops
    from video.analysis import curves
    a = np.asarray(curve)
    if ops.host_norm_is_pinned() or spacing is None:
        res = np.asarray(curves.make_curve_equidistant(a, spacing=spacing, count=count), np.float64)
        if offset is not None:
            res = curves.translate_points(res, offset[0], offset[1])
        return res
    return K.equidistant(a, spacing=spacing, count=count, offset=offset)


def _spy(monkeypatch, owner, name):
    """counts the calls of owner.name; returns the list the calls' positional arguments are appended to"""
    real, seen = getattr(owner, name), []

    def spied(*args, **kw):
        seen.append(args)
        return real(*args, **kw)
    monkeypatch.setattr(owner, name, spied)
    return seen


def _check(curves_, spacing=None, count=None, offsets=None):
    """ops.curves_equidistant against the per-curve function, the lengths against curve_length of the results"""
    from video import ops
    from video.analysis import curves
    m = len(curves_)
    got, lengths = ops.curves_equidistant(curves_, spacing, count, offsets, ret_lengths=True)
    assert len(got) == m and lengths.shape == (m,) and lengths.dtype == np.float64
    sps = spacing if isinstance(spacing, (list, tuple)) else [spacing] * m
    cts = count if isinstance(count, (list, tuple)) else [count] * m
    for k in range(m):
        want = _want(curves_[k], sps[k], None if sps[k] is not None else cts[k], None if offsets is None else offsets[k])
        assert got[k].dtype == np.float64 and bits_equal(got[k], want), (k, sps[k], cts[k])
        assert bits_equal([lengths[k]], [float(curves.curve_length(got[k]))]), k
    return got


# --------------------------------------------------------------------------------------- small shapes and edges
def test_point_counts_and_segments(gpu):
    two = np.array([[0., 0.], [100., 0.]])                      # many drops inside one segment
    slanted = np.array([[1.5, -2.25], [40.75, 33.5]])
    dup = np.array([[1., 1.], [1., 1.], [4., 5.]])              # a duplicate: a zero segment, equal s entries
    dup_end = np.array([[0., 0.], [3., 4.], [3., 4.]])
    same = np.full((5, 2), 3.25)                                # all points coincident: L = 0, s all 0
    batch = [two, slanted, dup, dup_end, same]
    for sp in (3, 0.7, 20, 1000):
        _check(batch, spacing=sp)
    for ct in (None, 1, 2, 7):
        _check(batch, count=ct)


def test_spacing_thresholds(gpu):
    ten = np.array([[0., 0.], [6., 8.]])                         # L = 10 exactly (float32 and double)
    below, above = float(np.nextafter(10.0, 11.0)), float(np.nextafter(10.0, 0.0))
    for sp in (below, 10.0, above):                              # L just below, equal to, just above the spacing
        _check([ten], spacing=sp)
    got = _check([ten, ten, ten], spacing=[below, 10.0, above])
    assert len(got[0]) == 2 and bits_equal(got[0], ten)          # L < spacing: the input
    _check([ten, np.array([[0., 0.], [14., 0.]])], spacing=4)    # L / spacing = 2.5 -> 2, 3.5 -> 4: half to even
    path = K.pixel_path(np.random.default_rng(3), 120)
    _check([path], spacing=20)                                   # larger than every segment
    _check([path], spacing=0.3)                                  # smaller than every segment


def test_result_counts_of_both_kinds(gpu):
    from video.analysis import curves
    cs = K.mixed_curves(21, 40, 5, 60)
    got = _check(cs, spacing=2.5)
    extra = {len(g) - int(np.round(curves.curve_length(c) / 2.5)) for g, c in zip(got, cs)
             if curves.curve_length(c) >= 2.5}
    assert {1, 2} <= extra                                       # rint(L / spacing) + 1 and + 2 both occur


def test_coordinate_kinds_and_fixture_curves(gpu):
    rng = np.random.default_rng(4)
    paths = [K.pixel_path(rng, n) for n in (2, 3, 17, 64, 150)]                  # int64 pixel paths
    far = [K.float_curve(rng, n, 1.5, 1000.0) for n in (2, 9, 80)]               # where the float32 casts bite
    inputs, z = K.fixture_curves()
    fixture = list(inputs.values())
    for batch in (paths, far, fixture):
        for kw in (dict(), dict(count=11), dict(spacing=2.5), dict(spacing=20)):
            _check(batch, **kw)
    from video import ops
    for name, pts in inputs.items():                                             # what the reference's code wrote
        assert bits_equal(ops.curves_equidistant([pts])[0], z["curves/%s/equidistant" % name])
        assert bits_equal(ops.curves_equidistant([pts], count=11)[0], z["curves/%s/equidistant_count" % name])
        assert bits_equal(ops.curves_equidistant([pts], spacing=2.5)[0], z["curves/%s/equidistant_spacing" % name])


def test_counts(gpu):
    cs = K.mixed_curves(5, 9, 2, 40)
    for ct in (1, 2):
        _check(cs, count=ct)
    _check(cs, count=[len(c) for c in cs])
    _check(cs, count=[4 * len(c) for c in cs])
    _check(cs, count=[1, 2, 3, None, 50, 7, None, 2, 1])                          # mixed per-curve counts
    _check(cs, spacing=[2.5, None, 0.7, None, 20, None, 5, None, 1.0], count=[None, 4, 9, None, 1, 3, 2, 2, 6])


@pytest.mark.parametrize("m", (1, 63, 64, 65, 257, 513))    # the offsets' scan takes 256 curves a round: 2 and 3 rounds
def test_batch_sizes(gpu, m):
    cs = K.mixed_curves(100 + m, m, 2, 300)
    rng = np.random.default_rng(m)
    offsets = [(int(a), int(b)) for a, b in rng.integers(-50, 50, (m, 2))]
    _check(cs, spacing=5)
    _check(cs, spacing=5, offsets=offsets)                                        # translations on and off
    _check(cs)
    _check(cs, count=13, offsets=offsets)


# --------------------------------------------------------------------------------------- the entry point
def _abi_run(L, curves_, spacing, counts, cap, fill=0xA5):
    """va_curves_equidistant on buffers of its own, the outputs filled with a byte before: the raw arrays"""
    from video import _hip
    arrs = [np.ascontiguousarray(c, np.float64) for c in curves_]
    m = len(arrs)
    off = np.concatenate([[0], np.cumsum([len(a) for a in arrs])]).astype(np.int64)
    bufs = dict(points=np.concatenate(arrs), off=off, sp=np.asarray(spacing, np.float64),
                ct=np.asarray(counts, np.int32))
    dev = {k: _hip.DeviceBuffer.from_array(v) for k, v in bufs.items()}
    outs = dict(count=(m, np.int32), out_off=(m + 1, np.int64), in_len=(m, np.float64), status=(m, np.int32),
                total=(1, np.int64), pts=(2 * max(cap, 1), np.float64), out_len=(m, np.float64))
    for k, (n, dt) in outs.items():
        dev[k] = _hip.DeviceBuffer(n * np.dtype(dt).itemsize)
        _hip.check(L.va_memset(dev[k].ptr, fill, dev[k].nbytes, None))
    _hip.check(L.va_curves_equidistant(dev["points"].ptr, dev["off"].ptr, int(off[-1]), m, dev["sp"].ptr, dev["ct"].ptr,
                                       None, dev["count"].ptr, dev["out_off"].ptr, dev["in_len"].ptr,
                                       dev["status"].ptr, dev["total"].ptr, dev["pts"].ptr, cap, dev["out_len"].ptr,
                                       None))
    res = {k: dev[k].download((n,), dt) for k, (n, dt) in outs.items()}
    for b in dev.values():
        b.free()
    return res


def test_overflow_is_reported_and_nothing_written(gpu):
    from video.analysis import curves
    cs = [np.asarray(c, np.float64) for c in K.mixed_curves(31, 20, 2, 60)]
    sp = [2.5 if k % 2 else 0.0 for k in range(20)]
    ct = [0 if k % 2 else 9 for k in range(20)]
    want = [_want(c, spacing=2.5) if k % 2 else _want(c, count=9) for k, c in enumerate(cs)]
    total = sum(len(w) for w in want)
    short = _abi_run(gpu, cs, sp, ct, total - 1)
    assert short["total"][0] == total and np.array_equal(short["count"], [len(w) for w in want])
    assert np.all(short["pts"].view(np.uint8) == 0xA5)                         # too small by one point: none written
    assert np.all(short["out_len"] == 0) and np.all(short["status"] == 0)
    full = _abi_run(gpu, cs, sp, ct, total)
    assert full["total"][0] == total and bits_equal(full["pts"].reshape(-1, 2), np.concatenate(want))
    assert np.array_equal(full["out_off"], np.concatenate([[0], np.cumsum([len(w) for w in want])]))
    for k, c in enumerate(cs):
        assert bits_equal([full["in_len"][k]], [curves.curve_length(c)]) or not k % 2
        assert bits_equal([full["out_len"][k]], [curves.curve_length(want[k])])
    again = _abi_run(gpu, cs, sp, ct, total, fill=0x00)                         # two runs: identical bytes
    for key in full:
        assert full[key].tobytes() == again[key].tobytes(), key


def test_refused_curves_leave_the_others(gpu):
    line = np.array([[0., 0.], [3., 4.], [6., 8.]])
    res = _abi_run(gpu, [line, line[:1], line, line, line], [2.5, 2.5, -1.0, 0.0, 1e-9], [0, 0, 0, 0, 0], 64)
    assert res["status"].tolist() == [0, -34, -34, -34, -34]                   # one point; bad spacing; count 0; steps
    assert res["count"].tolist() == [len(_want(line, spacing=2.5)), 0, 0, 0, 0]
    assert bits_equal(res["pts"][:2 * res["count"][0]].reshape(-1, 2), _want(line, spacing=2.5))
    assert np.all(res["pts"][2 * res["count"][0]:].view(np.uint8) == 0xA5)


def test_retry_through_ops(gpu, monkeypatch):
    from video import _hip, ops

    class Counting(object):
        """the library with its va_curves_equidistant calls counted: (capacity asked for) of each"""
        caps = []

        def __getattr__(self, name):
            fn = getattr(gpu, name)
            if name != "va_curves_equidistant":
                return fn

            def counted(*args):
                self.caps.append(args[13])
                return fn(*args)
            return counted
    proxy = Counting()
    monkeypatch.setattr(_hip, "lib", lambda device=None: proxy)
    cs = K.mixed_curves(41, 12, 20, 60)
    want = ops.curves_equidistant(cs, spacing=0.5)
    total = sum(len(w) for w in want)
    assert len(proxy.caps) == 1 and proxy.caps[0] >= total                    # the estimate had room: one launch
    del proxy.caps[:]
    monkeypatch.setattr(ops, "CURVES_ROOM_SLACK", -10 ** 6)                    # the first launch has too little room
    got = ops.curves_equidistant(cs, spacing=0.5)
    assert len(proxy.caps) == 2 and proxy.caps[0] < total and proxy.caps[1] == total      # once more, with exact room
    for g, w, c in zip(got, want, cs):
        assert bits_equal(g, w) and bits_equal(g, _want(c, spacing=0.5))


@pytest.mark.parametrize("fill", (0xFF, 0xA5))
def test_on_filled_memory_with_guarded_tails(gpu, fill):
    from video import _hip, ops
    cs = K.mixed_curves(51, 70, 2, 90)
    offsets = [(k - 30, 2 * k) for k in range(70)]
    ops.pool_clear()
    _hip.set_fill_mode(fill)
    try:
        for _ in (1, 2):                                                       # the second call gets recycled buffers
            _check(cs, spacing=2.5, offsets=offsets)
            _check(cs, count=11)
        found = _hip.check_guards()
    finally:
        _hip.set_fill_mode(-1)
        ops.pool_clear()
        _hip.check_guards()
    assert found == [], found


# --------------------------------------------------------------------------------------- public functions, callers
def test_public_function_equals_the_per_curve_one(gpu):
    from video import ops
    from video.analysis import curves
    m = max(ops.CURVES_DEVICE_MIN_BATCH, 12)
    cs = K.mixed_curves(61, m, 2, 80)
    for kw in (dict(), dict(count=11), dict(spacing=2.5), dict(count=[k + 1 for k in range(m)])):
        got = curves.make_curves_equidistant(cs, **kw)
        for k, (g, c) in enumerate(zip(got, cs)):
            one = {key: (v[k] if isinstance(v, list) else v) for key, v in kw.items()}
            assert bits_equal(g, _want(c, one.get("spacing"), one.get("count"))), (kw, k)
    few = curves.make_curves_equidistant(cs[:1], spacing=2.5)                   # below the threshold: the same bits
    assert bits_equal(few[0], _want(cs[0], spacing=2.5))


def test_find_contours_on_a_batch_equals_find_contour(gpu, monkeypatch):
    from video import ops
    assert ops.host_norm_is_pinned()                                           # else the callers stay on the host
    calls = _spy(monkeypatch, ops, "curves_equidistant")
    from video.analysis.active_contour import ActiveContour
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[:96, :128]
    stack = np.stack([np.exp(-((xx - 64 - 9 * f) ** 2 + (yy - 48) ** 2) / 900.0).astype(np.float32) * 200
                      for f in range(3)])
    m = max(ops.CURVES_DEVICE_MIN_BATCH, 10)
    cs = [K.float_curve(rng, int(rng.integers(2, 40)), 2.0, 0.0) + (60, 45) for _ in range(m)]
    cs[1] = cs[1][:2]                                                          # two points: comes back untouched
    frames = [k % 3 for k in range(m)]
    anchors = [None if k % 2 else [0, len(c) - 1] for k, c in enumerate(cs)]
    ac = ActiveContour(blur_radius=2, alpha=0.1, beta=10.0, gamma=0.01)
    ac.max_iterations = 30
    ac.set_potential(stack)
    got = ac.find_contours(cs, frames, anchors, anchors)
    assert len(calls) == 1 and len(calls[0][0]) == m                           # one device call for the whole batch
    its, tvs = ac.info["iteration_count"].copy(), ac.info["total_variation"].copy()
    for k, c in enumerate(cs):
        one = ac.find_contour(c, anchors[k], anchors[k], frame=frames[k])
        assert bits_equal(got[k], one), k
        assert len(calls) == 1                                                 # (one curve: below the threshold)
        if len(one) > 2:
            assert its[k] == ac.info["iteration_count"] and tvs[k] == ac.info["total_variation"], k


def test_centerlines_equal_the_per_polygon_method(gpu, monkeypatch):
    from video import ops
    assert ops.host_norm_is_pinned()
    from video.analysis.shapes import Polygon, get_centerlines_optimized
    spec = importlib.util.spec_from_file_location("make_golden_polygon",
                                                  os.path.join(ROOT, "tests", "golden", "make_golden_polygon.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    names = [n for n in ("worm", "worm_steep", "mouse", "u_shape", "l_shape") if n in G.FILL_POLYS]
    assert len(names) >= 4
    params = dict(alpha=10., beta=100., gamma=0.01, spacing=5, max_iterations=60)
    single = {n: Polygon(G.FILL_POLYS[n]).get_centerline_optimized(**params) for n in names}
    m = max(ops.CURVES_DEVICE_MIN_BATCH, len(names))
    batch = [names[k % len(names)] for k in range(m)]                          # enough polygons for the device path
    calls = _spy(monkeypatch, ops, "curves_equidistant")
    got = get_centerlines_optimized([Polygon(G.FILL_POLYS[n]) for n in batch], **params)
    assert len(calls) == 3                     # the estimates, the curves inside find_contours, the found contours
    assert all(isinstance(g, np.ndarray) and g.dtype == np.float64 for g in got)
    for n, g in zip(batch, got):
        assert bits_equal(g, single[n]), n
