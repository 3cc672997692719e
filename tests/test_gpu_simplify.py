"""GPU: the batched simplifiers (va_simplify_rdp, va_simplify_visvalingam, ops.simplify_curves,
curves.simplify_curves, regions.simplify_contours, get_morphological_graphs(batched_simplify=True)) against the
scalar restatements of tests/simplify_checks.py ("Simplification"): flags, counts and statuses, byte
for byte.  The whole module runs in the test fill mode (video._hip.set_fill_mode, as tests/test_gpu_hostile_memory.py
uses it): every buffer, the workspace included, holds 0xA5 before a call and has a guarded tail behind it."""
import importlib.util
import os

import numpy as np
import pytest

import simplify_checks as K

pytestmark = pytest.mark.gpu

ROOT = K.ROOT
MODES = (("rdp", False), ("visvalingam", True), ("visvalingam", False))
TOLERANCES = (0, 0.1, 0.5, 1, 2, 10, 200, 1e9)


@pytest.fixture(scope="module", autouse=True)
def dirty():
    """0xA5 in every device buffer of this module's calls, guarded tails checked at the end"""
    from video import _hip, ops
    _hip.lib()
    ops.pool_clear()
    _hip.set_fill_mode(0xA5)
    try:
        yield
        found = _hip.check_guards()
    finally:
        _hip.set_fill_mode(-1)
        ops.pool_clear()
        _hip.check_guards()
    assert found == [], found


def _abi_run(method, closed, curves_, tol, point_off=None):
    """one call on buffers of its own: dict of the raw keep, count and status arrays.  Outputs and workspace start
    out as 0xA5 (the fill mode) and every buffer's guarded tail is checked when it is freed"""
    from video import _hip
    L = _hip.lib()
    arrs = [np.ascontiguousarray(c, np.float64).reshape(-1, 2) for c in curves_]
    m = len(arrs)
    off = np.concatenate([[0], np.cumsum([len(a) for a in arrs])]).astype(np.int64)
    npoints = int(off[-1])
    if point_off is not None:
        off = np.asarray(point_off, np.int64)
    points = np.concatenate(arrs + [np.zeros((1, 2))])                      # (one spare row: never an empty upload)
    dev = {k: _hip.DeviceBuffer.from_array(v) for k, v in
           dict(points=points, off=off, tol=np.asarray(tol, np.float64)).items()}
    outs = dict(keep=(npoints, np.uint8), count=(m, np.int32), status=(m, np.int32))
    for k, (n, dt) in outs.items():
        dev[k] = _hip.DeviceBuffer(max(n, 1) * np.dtype(dt).itemsize)
    if method == "rdp":
        _hip.check(L.va_simplify_rdp(dev["points"].ptr, dev["off"].ptr, npoints, m, dev["tol"].ptr, dev["keep"].ptr,
                                     dev["count"].ptr, dev["status"].ptr, None))
    else:
        need = L.va_simplify_visvalingam_workspace_bytes(npoints)
        dev["ws"] = _hip.DeviceBuffer(need)
        _hip.check(L.va_simplify_visvalingam(dev["points"].ptr, dev["off"].ptr, npoints, m, dev["tol"].ptr,
                                             int(closed), dev["keep"].ptr, dev["count"].ptr, dev["status"].ptr,
                                             dev["ws"].ptr, need, None))
    res = {k: dev[k].download((n,), dt) for k, (n, dt) in outs.items()}
    for b in dev.values():
        b.free()
    assert _hip.check_guards() == []
    return res


def _restated(method, closed, curve, tol):
    return K.rdp_keep(curve, tol) if method == "rdp" else K.visvalingam_keep(curve, tol, closed)


def _check(method, closed, curves_, tol, want=None):
    """the raw call against the restatement (or the flags given): flags, counts, statuses; returns the raw arrays"""
    m = len(curves_)
    tol = [tol] * m if np.ndim(tol) == 0 else list(tol)
    if want is None:
        want = [_restated(method, closed, c, t) for c, t in zip(curves_, tol)]
    res = _abi_run(method, closed, curves_, tol)
    assert res["status"].tolist() == [0] * m
    assert res["count"].tolist() == [int(w.sum()) for w in want]
    flags = np.concatenate(want + [np.zeros(0, np.uint8)])
    assert res["keep"].tobytes() == flags.astype(np.uint8).tobytes()
    return res


# --------------------------------------------------------------------------------------- fixtures
def test_fixture_entries_equal_the_restatement_and_the_reference():
    for closed in (True, False):
        cases = [c for c in K.fixture() if c[2] == closed]
        res = _check("visvalingam", closed, [c[1] for c in cases], [c[3] for c in cases])
        at = 0
        for name, curve, _, thr, want in cases:                      # ... and what the reference's own code returned
            keep = res["keep"][at:at + len(curve)].astype(bool)
            at += len(curve)
            assert K.same_result(None if closed and not keep.any() else curve[keep], want), (name, thr)
    cases = K.rdp_fixture()
    res = _check("rdp", False, [c[1] for c in cases], [c[2] for c in cases])
    at = 0
    for name, curve, eps, want in cases:
        assert K.same_result(curve[res["keep"][at:at + len(curve)].astype(bool)], want), (name, eps)
        at += len(curve)
    rings = [c[1] for c in K.fixture()[::6]]
    for eps in (0, 0.5, 2):
        _check("rdp", False, rings, eps)


# --------------------------------------------------------------------------------------- shapes
@pytest.fixture(scope="module")
def mixed():
    """curves of 0 .. 129 points, six of each length and of mixed kinds, and one of 2080 (longer than the 2048
    points the RDP kernel stages in LDS), shuffled so that a wave holds curves of unequal length; one tolerance per
    curve; the restated flags of the three modes, computed once"""
    rng = np.random.default_rng(2080)
    curves_ = [K.random_curve(rng, n) for n in (0, 1, 2, 3, 4, 63, 64, 65, 128, 129) for _ in range(6)]
    curves_.append(K.noisy_circle(rng, 2080))
    order = rng.permutation(len(curves_))
    curves_ = [curves_[k] for k in order]
    tol = [TOLERANCES[int(rng.integers(len(TOLERANCES)))] if len(c) < 2000 else 0.4 for c in curves_]
    want = {mode: [_restated(mode[0], mode[1], c, t) for c, t in zip(curves_, tol)] for mode in MODES}
    return curves_, tol, want


@pytest.mark.parametrize("mode", range(len(MODES)))
def test_mixed_lengths_and_tolerances(mixed, mode):
    curves_, tol, want = mixed
    method, closed = MODES[mode]
    first = _check(method, closed, curves_, tol, want[MODES[mode]])
    again = _abi_run(method, closed, curves_, tol)                               # two runs: identical bytes
    for key in first:
        assert first[key].tobytes() == again[key].tobytes(), key
    counts = first["count"]
    long_one = [k for k, c in enumerate(curves_) if len(c) == 2080][0]
    assert 2 < counts[long_one] < 2080                                           # the long curve was really thinned


@pytest.mark.parametrize("mode", range(len(MODES)))
def test_one_curve(mixed, mode):
    curves_, tol, want = mixed
    method, closed = MODES[mode]
    for k in [k for k, c in enumerate(curves_) if len(c) in (0, 2, 3, 65)][:8]:
        _check(method, closed, [curves_[k]], [tol[k]], [want[MODES[mode]][k]])


@pytest.mark.parametrize("mode", range(len(MODES)))
def test_more_curves_than_one_launch_of_65535(mode):
    """70 000 curves of 3 .. 5 points: 500 distinct ones, restated once each, in a seeded order"""
    method, closed = MODES[mode]
    rng = np.random.default_rng(70000)
    distinct = [K.random_curve(rng, int(rng.integers(3, 6))) for _ in range(500)]
    tol = [(0, 0.3, 0.5, 1.0, 2.0)[int(rng.integers(5))] for _ in distinct]
    flags = [_restated(method, closed, c, t) for c, t in zip(distinct, tol)]
    pick = rng.integers(0, 500, 70000)
    pick[-3:] = (7, 8, 9)
    res = _check(method, closed, [distinct[k] for k in pick], [tol[k] for k in pick], [flags[k] for k in pick])
    assert len(set(res["count"][65535:].tolist())) > 1


def test_rdp_parabola_peels_one_point_a_split():
    """1000 points on a parabola, eps = 0: the farthest point of every span is its second, so the spans stack up"""
    x = np.arange(1000, dtype=np.float64)
    res = _check("rdp", False, [np.stack([x, x * x], 1), np.stack([x[::-1], x * x], 1)], 0)
    assert res["count"].tolist() == [1000, 1000]


def test_rdp_loop_with_equal_ends_and_vertical_chords():
    rng = np.random.default_rng(5)
    loops = []
    for n in (5, 40, 200):
        ring = K.noisy_circle(rng, n)
        loops.append(np.concatenate([ring, ring[:1]]))                           # equal ends: |x0.x - x1.x|
    loops.append(np.array([[2., 1.], [5., 1.], [5., 4.], [2., 4.], [2., 1.]]))
    loops.append(np.array([[3, 0], [3, 5], [4, 9], [3, 12], [3, 20]], np.int64))  # a vertical chord with distinct ends
    loops.append(np.full((70, 2), 3.25))                                         # every point the same
    for eps in (0, 0.5, 3, 1e9):
        _check("rdp", False, loops, eps)


def test_rdp_longer_than_the_staging_limit():
    rng = np.random.default_rng(6)
    curves_ = [K.float_walk(rng, 2049), K.staircase(rng, 5000), K.float_walk(rng, 2048)]
    res = _check("rdp", False, curves_, [1.5, 0.9, 1.5])
    assert all(2 < c < len(p) for c, p in zip(res["count"], curves_))


def test_visvalingam_everything_below_and_everything_above():
    rng = np.random.default_rng(7)
    rings = [K.noisy_circle(rng, n) for n in (3, 4, 50, 129)] + [K.integer_contour(rng, 64)]
    below = _check("visvalingam", True, rings, 1e9)
    assert below["count"].tolist() == [0] * 5 and not below["keep"].any()         # every ring vanishes: None
    lines = _check("visvalingam", False, rings, 1e9)
    assert lines["count"].tolist() == [2] * 5                                    # a line keeps its two ends
    spiky = [np.stack([np.arange(n), 50.0 * (np.arange(n) % 2)], 1) for n in (3, 4, 50, 129)]
    above = _check("visvalingam", True, spiky, 1.0)
    assert above["count"].tolist() == [3, 4, 50, 129] and above["keep"].all()     # nothing is removed
    assert _check("visvalingam", False, spiky, 1.0)["keep"].all()


def test_curves_that_are_not_run_leave_the_others():
    line = np.array([[0., 0.], [3., 4.], [6., 8.], [7., 0.], [9., 1.]])
    for method, closed in MODES:
        want = _restated(method, closed, line, 0.5)
        res = _abi_run(method, closed, [line] * 4, [0.5, float("nan"), 0.5, 0.5], point_off=[0, 5, 10, 25, 20])
        assert res["status"].tolist() == [0, -34, -34, -34]                      # NaN; beyond the buffer; out of order
        assert res["count"].tolist() == [int(want.sum()), 0, 0, 0]
        assert res["keep"][:5].tolist() == want.tolist() and not res["keep"][5:10].any()
        assert np.all(res["keep"][10:] == 0xA5)                                  # slots of no curve: untouched


# --------------------------------------------------------------------------------------- the layers above
def test_ops_and_the_reference_named_functions(mixed, monkeypatch):
    from video import ops
    from video.analysis import curves, regions
    curves_, tol, want = mixed
    short = [k for k, c in enumerate(curves_) if len(c) < 200]
    cs, ts = [curves_[k] for k in short], [tol[k] for k in short]
    assert len(cs) >= ops.SIMPLIFY_DEVICE_MIN_BATCH
    calls = []
    real = ops._simplify_on_host
    monkeypatch.setattr(ops, "_simplify_on_host", lambda *a: calls.append(a) or real(*a))
    for method, closed in MODES:
        got = ops.simplify_curves(cs, ts, method=method, closed=closed)
        for j, k in enumerate(short):
            keep = want[(method, closed)][k].astype(bool)
            expect = None if closed and not keep.any() else np.asarray(cs[j])[keep]
            assert K.same_result(got[j], expect), (method, closed, k)
    assert all(len(a[0]) == 0 for a in calls)                                    # only the empty curves stayed behind
    got = curves.simplify_curves(cs, 0.5)
    assert all(K.same_result(g, K.simplified(c, 0.5)) for g, c in zip(got, cs))
    # a NaN tolerance and a non-finite point stay on the host, inside a batch that goes to the device
    nan = np.array([[0., 0.], [np.nan, 1.], [2., 2.], [3., 0.]])
    got = ops.simplify_curves(cs[:10] + [nan], ts[:9] + [float("nan"), 0.5])
    assert K.same_result(got[9], K.simplified(cs[9], float("nan"))) and K.same_result(got[10], K.simplified(nan, 0.5))
    ring = next(c for c in cs if len(c) >= 60)
    assert K.same_result(regions.simplify_contour(ring, 1.0), K.simplified(ring, 1.0, "visvalingam", True))


def test_simplify_contours_of_find_contours():
    from video import ops
    from video.analysis import regions
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[:72, :96]
    masks = np.zeros((3, 72, 96), np.uint8)
    for f in range(3):
        for _ in range(6):
            cx, cy, r = rng.integers(8, 88), rng.integers(8, 64), rng.integers(3, 14)
            masks[f][(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = 1
    found = ops.find_contours(masks)
    assert sum(len(f) for f in found) >= ops.SIMPLIFY_DEVICE_MIN_BATCH
    for thr in (0.5, 2):
        got = regions.simplify_contours(found, thr)
        assert [len(g) for g in got] == [len(f) for f in found]
        for frame, res in zip(found, got):
            for contour, g in zip(frame, res):
                assert K.same_result(g, K.simplified(contour.reshape(-1, 2), thr, "visvalingam", True))
    flat = [c for f in found for c in f]
    lines = regions.simplify_contours(flat, 2, closed=False)
    assert all(K.same_result(g, K.simplified(c.reshape(-1, 2), 2, "visvalingam", False)) for g, c in zip(lines, flat))


def _thinning():
    spec = importlib.util.spec_from_file_location(
        "make_golden_skeleton_graph", os.path.join(ROOT, "tests", "golden", "make_golden_skeleton_graph.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.thinning()


def _same_graph(g, w, name):
    assert list(g.nodes(data=True)) == list(w.nodes(data=True)), name
    ge, we = list(g.edges(keys=True, data=True)), list(w.edges(keys=True, data=True))
    assert len(ge) == len(we), name
    for (a1, b1, k1, d1), (a2, b2, k2, d2) in zip(ge, we):
        assert (a1, b1, k1) == (a2, b2, k2) and d1["length"] == d2["length"], name
        assert K.same_result(d1["curve"], d2["curve"]), name


def test_morphological_graphs_batched_and_default(monkeypatch):
    from video import ops
    from video.analysis import curves, shapes
    T = _thinning()
    polys = [shapes.Polygon(T.POL.FILL_POLYS[name]) for name in T.POLYGONS]
    # the default call is what it was: the per-polygon method
    for name, poly, g in zip(T.POLYGONS, polys, shapes.get_morphological_graphs(polys)):
        _same_graph(g, poly.get_morphological_graph(), name)
    # batched: the merged, translated graphs with every curve through the restatement (integer curves: a translation
    # by integers changes no distance, so thinning before or after it keeps the same points)
    want = shapes.get_morphological_graphs(polys, simplify_epsilon=0)
    edges = sum(g.number_of_edges() for g in want)
    monkeypatch.setattr(ops, "SIMPLIFY_DEVICE_MIN_BATCH", min(ops.SIMPLIFY_DEVICE_MIN_BATCH, edges))
    for g in want:
        for _, _, data in g.edges(data=True):
            data["curve"] = K.simplified(data["curve"], 0.1)
            data["length"] = curves.curve_length(data["curve"])
    got = shapes.get_morphological_graphs(polys, simplify_epsilon=0.1, batched_simplify=True)
    for name, g, w in zip(T.POLYGONS, got, want):
        _same_graph(g, w, name)
    raw = shapes.get_morphological_graphs(polys, simplify_epsilon=0, batched_simplify=True)
    for name, g, w in zip(T.POLYGONS, raw, shapes.get_morphological_graphs(polys, simplify_epsilon=0)):
        _same_graph(g, w, name)
