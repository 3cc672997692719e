"""CPU: the two pinned simplifiers ("Simplification").  The restatements of tests/simplify_checks.py
equal what the reference's own code returned -- simplify_ring and simplify_line on tests/golden/simplify_v1.npz, rdp
on the 27 rdp/* entries of tests/golden/skeleton_graph_v1.npz; va_simplify_math.h, compiled with the host compiler,
equals the restatements on the fixtures and on 500 seeded random curves, for distances, areas, kept sets and heap
order; the entry points are declared and bound; the public functions check their arguments and route small
batches through the definition in Python.  Comparisons are exact."""
import os

import numpy as np
import pytest

import simplify_checks as K

ROOT = K.ROOT


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = K.compile_shim(tmp_path_factory.mktemp("simplify_shim"))
    if lib is None:
        pytest.skip("no host C++ compiler")
    return lib


@pytest.fixture(scope="module")
def random_cases():
    """500 seeded curves of 3..120 points with a tolerance each: (curve, tolerance)"""
    rng = np.random.default_rng(77)
    tolerances = (0, 0.1, 0.5, 1, 2, 10, 200, 1e9)
    return [(c, tolerances[int(rng.integers(len(tolerances)))]) for c in K.random_curves(78, 500)]


# ------------------------------------------------------------------------------------------- the restatements
def test_visvalingam_restatement_equals_the_reference_on_every_fixture_entry():
    cases = K.fixture()
    assert len(cases) >= 6 * 40 and len({name for name, _, _, _, _ in cases}) >= 38
    vanished = kept_all = 0
    for name, curve, closed, thr, want in cases:
        got = K.simplified(curve, thr, "visvalingam", closed)
        assert K.same_result(got, want), (name, closed, thr)
        vanished += want is None
        kept_all += want is not None and len(want) == len(curve)
    assert vanished >= 10 and kept_all >= 10
    assert {thr for _, _, _, thr, _ in cases} == set(float(t) for t in K.THRESHOLDS)


def test_rdp_restatement_equals_the_reference_rdp_entries():
    cases = K.rdp_fixture()
    assert len(cases) == 27
    for name, curve, eps, want in cases:
        assert K.same_result(K.simplified(curve, eps, "rdp"), want), (name, eps)


def test_rdp_edges_of_the_definition():
    loop = np.array([[2., 1.], [5., 1.], [5., 4.], [2., 4.], [2., 1.]])          # equal ends: |x0.x - x1.x|
    assert K.span_farthest(loop.tolist(), 0, 4) == (3.0, 1)                       # the first of the two largest
    assert K.rdp_keep(loop, 3).tolist() == [1, 0, 0, 0, 1] and K.rdp_keep(loop, 2.9).tolist() == [1, 1, 1, 0, 1]
    tie = np.array([[0, 0], [1, 2], [2, -2], [3, 2], [4, 0]])
    assert K.rdp_keep(tie, 0).tolist() == [1, 1, 1, 1, 1] and K.rdp_keep(tie, 1.9).tolist() == [1, 1, 1, 1, 1]
    assert K.rdp_keep(tie, 2).tolist() == [1, 0, 0, 0, 1]                         # d == eps does not split
    assert K.rdp_keep(tie, -5).tolist() == [1, 1, 1, 1, 1]                        # max(eps, 0)
    flat = np.array([[0, 0], [1, 0], [2, 0], [3, 0]])
    assert K.rdp_keep(flat, 0).tolist() == [1, 0, 0, 1]                           # d == 0 never splits
    for n in (0, 1, 2):
        assert K.rdp_keep(np.zeros((n, 2)), 0).tolist() == [1] * n


# ------------------------------------------------------------------------------------------- the math header
def test_header_distances_and_areas(shim, random_cases):
    rows = []
    for curve, _ in random_cases[:120]:
        P = np.asarray(curve, np.float64)
        for i in range(1, len(P) - 1):
            rows.append(np.concatenate([P[i], P[0], P[-1]]))
            rows.append(np.concatenate([P[i], P[i - 1], P[i + 1]]))
            rows.append(np.concatenate([P[i], P[i - 1], [P[i - 1][0], P[i + 1][1]]]))      # chord ends of equal x
    rows = np.ascontiguousarray(rows, np.float64)
    assert len(rows) > 10000
    dist, area = np.empty(len(rows)), np.empty(len(rows))
    shim.ss_chord_distance(rows.ctypes.data, dist.ctypes.data, len(rows))
    shim.ss_triangle_area(rows.ctypes.data, area.ctypes.data, len(rows))
    want_d = np.array([K.chord_distance(r[0:2], r[2:4], r[4:6]) for r in rows.tolist()])
    want_a = np.array([K.triangle_area(r[0:2], r[2:4], r[4:6]) for r in rows.tolist()])
    assert dist.tobytes() == want_d.tobytes() and area.tobytes() == want_a.tobytes()


def test_header_span_step_is_independent_of_the_lanes(shim, random_cases):
    import ctypes as C
    for curve, _ in random_cases[:150]:
        P = np.ascontiguousarray(curve, np.float64)
        want_d, want_i = K.span_farthest(P.tolist(), 0, len(P) - 1)
        for lanes in (1, 7, 64):
            d = C.c_double()
            index = shim.ss_span_farthest(P.ctypes.data, 0, len(P) - 1, lanes, C.byref(d))
            assert d.value == want_d and index == (want_i if want_i is not None else 0x7FFFFFFF)


def _check_header(shim, curve, tol, closed_modes=(False, True)):
    keep, count = K.shim_rdp(shim, curve, tol)
    want = K.rdp_keep(curve, tol)
    assert keep.tolist() == want.tolist() and count == int(want.sum())
    for closed in closed_modes:
        keep, count, heap = K.shim_visvalingam(shim, curve, tol, closed)
        want, want_heap = K.visvalingam(curve, tol, closed)
        assert keep.tolist() == want.tolist() and count == int(want.sum()), (closed, tol)
        assert heap == want_heap, (closed, tol)                                   # the heap, entry by entry


def test_header_equals_the_restatement_on_the_fixtures(shim):
    for name, curve, closed, thr, want in K.fixture():
        _check_header(shim, curve, thr, (closed,))
        keep, _, _ = K.shim_visvalingam(shim, curve, thr, closed)
        assert K.same_result(None if closed and not keep.any() else curve[keep.astype(bool)], want), (name, thr)
    for name, curve, eps, want in K.rdp_fixture():
        keep, count = K.shim_rdp(shim, curve, eps)
        assert K.same_result(curve[keep.astype(bool)], want) and count == len(want), (name, eps)


def test_header_equals_the_restatement_on_random_curves(shim, random_cases):
    assert len(random_cases) == 500
    for curve, tol in random_cases:
        _check_header(shim, curve, tol)
    for n in (0, 1, 2):                                                           # shorter than the algorithms need
        _check_header(shim, np.arange(2 * n, dtype=np.float64).reshape(n, 2), 1.0)
    x = np.arange(1000, dtype=np.float64)
    _check_header(shim, np.stack([x, x * x], 1), 0, ())                           # every split peels one point


# ------------------------------------------------------------------------------------------- the layers
def test_entry_points_are_declared_and_bound():
    from video import _hip
    text = open(os.path.join(ROOT, "include", "videoanalysis_hip.h")).read()
    assert "int va_simplify_rdp(" in text and "int va_simplify_visvalingam(" in text
    assert "regions.py:307-325" in text and "curves.py:22" in text and "VA_SIMPLIFY_MAX_POINTS" in text
    assert len(_hip.SIGNATURES["va_simplify_rdp"][1]) == 9
    assert len(_hip.SIGNATURES["va_simplify_visvalingam"][1]) == 12
    lib = _hip.load_library()
    # argument checks run before anything touches a device
    assert lib.va_simplify_rdp(None, None, -1, 1, None, None, None, None, None) == -22
    assert lib.va_simplify_rdp(None, None, 0, 1, None, None, None, None, None) == -22
    assert b"NULL" in lib.va_last_error()
    assert lib.va_simplify_rdp(None, None, 0, 0, None, None, None, None, None) == 0
    assert lib.va_simplify_visvalingam(None, None, 0, 0, None, 2, None, None, None, None, 0, None) == -22
    assert lib.va_simplify_visvalingam(None, None, 0, 0, None, 1, None, None, None, None, 0, None) == 0
    assert lib.va_simplify_visvalingam(None, None, 0, 1, None, 1, None, None, None, None, 0, None) == -22
    assert lib.va_simplify_visvalingam_workspace_bytes(1000) >= 12000
    assert lib.va_simplify_visvalingam_workspace_bytes(0) == 0 or lib.va_simplify_visvalingam_workspace_bytes(0) % 256 == 0


def test_small_batches_take_the_definition_in_python(random_cases):
    """below ops.SIMPLIFY_DEVICE_MIN_BATCH no GPU is touched; the results are the restatement's, in the input's
    dtype"""
    from video import ops
    from video.analysis import curves, regions
    assert ops.SIMPLIFY_DEVICE_MIN_BATCH >= 2
    for curve, tol in random_cases[:40]:
        assert K.same_result(ops.simplify_curves([curve], tol)[0], K.simplified(curve, tol, "rdp"))
        assert K.same_result(curves.simplify_curves([curve], tol)[0], K.simplified(curve, tol, "rdp"))
        for closed in (False, True):
            got = ops.simplify_curves([curve], tol, method="visvalingam", closed=closed)[0]
            assert K.same_result(got, K.simplified(curve, tol, "visvalingam", closed)), (tol, closed)
        assert K.same_result(regions.simplify_contour(curve, tol), K.simplified(curve, tol, "visvalingam", True))
    for name, curve, closed, thr, want in K.fixture()[::7]:
        assert K.same_result(regions.simplify_contours([curve], thr, closed=closed)[0], want), (name, thr)
    as_f32 = np.array([[0, 0], [1, 0.01], [2, 0], [3, 5]], np.float32)
    assert ops.simplify_curves([as_f32], 0.5)[0].dtype == np.float32
    assert ops.simplify_curves([], 1.0) == []
    # what the device does not take stays on the host whatever the batch size
    nan = np.array([[0., 0.], [np.nan, 1.], [2., 2.], [3., 0.]])
    huge = np.array([[0, 0], [2 ** 53, 1], [5, 5]], np.int64)
    empty = np.zeros((0, 2))
    got = ops.simplify_curves([nan, huge, empty] * ops.SIMPLIFY_DEVICE_MIN_BATCH, 0.5)
    assert K.same_result(got[0], K.simplified(nan, 0.5)) and K.same_result(got[1], K.simplified(huge, 0.5))
    assert got[2].shape == (0, 2)
    got = ops.simplify_curves([nan, empty], float("nan"), method="visvalingam", closed=True)
    assert got == [None, None]


def test_argument_checks(monkeypatch):
    from video import ops
    from video.analysis import curves, regions
    line = np.array([[0., 0.], [3., 4.], [6., 8.], [7., 0.]])
    with pytest.raises(ValueError, match="method"):
        ops.simplify_curves([line], 1.0, method="reumann")
    with pytest.raises(ValueError, match="open"):
        ops.simplify_curves([line], 1.0, method="rdp", closed=True)
    with pytest.raises(ValueError, match="tolerance"):
        ops.simplify_curves([line, line], [1.0])
    with pytest.raises(ValueError, match="tolerance"):
        ops.simplify_curves([line], None)
    with pytest.raises(ValueError, match="curve 1 has shape"):
        ops.simplify_curves([line, np.zeros((4, 3))], 1.0)
    # the reference-named functions, with the device call replaced: what reaches it, and what they make of its answer
    seen = []

    def fake(curves_, tolerance, method="rdp", closed=False, stream=None):
        seen.append(([np.asarray(c) for c in curves_], tolerance, method, closed))
        return [None if k % 2 else np.asarray(c)[:1] for k, c in enumerate(curves_)]
    monkeypatch.setattr(ops, "simplify_curves", fake)
    assert len(curves.simplify_curves([line, line], 0.3)) == 2 and seen[-1][1:] == (0.3, "rdp", False)
    closed_ring = np.concatenate([line, line[:1]])
    assert regions.simplify_contour(closed_ring, 2.5).shape == (1, 2)
    assert seen[-1][1:] == (2.5, "visvalingam", True) and np.array_equal(seen[-1][0][0], line)   # duplicate dropped
    cv = [line.astype(np.int32).reshape(-1, 1, 2), closed_ring.astype(np.int32).reshape(-1, 1, 2)]
    got = regions.simplify_contours(cv, 1.0)                                        # find_contours' own layout
    assert [c.shape for c in seen[-1][0]] == [(4, 2), (4, 2)] and got[1] is None
    got = regions.simplify_contours([cv, [], cv[:1]], 1.0)                          # a stack: one list per frame
    assert [len(g) for g in got] == [2, 0, 1] and [c.shape for c in seen[-1][0]] == [(4, 2), (4, 2), (4, 2)]
    regions.simplify_contours(cv, 1.0, closed=False)
    assert seen[-1][3] is False and seen[-1][0][1].shape == (5, 2)                  # a line keeps its last point
    with pytest.raises(ValueError, match="at least 3"):
        regions.simplify_contour(line[:2], 1.0)
    with pytest.raises(ValueError, match="at least 3"):
        regions.simplify_contour(np.array([[0, 0], [1, 1], [0, 0]]), 1.0)
    with pytest.raises(ValueError, match="shape"):
        regions.simplify_contour(np.zeros((5, 3)), 1.0)

    class LinearRing(object):
        coords = [(0, 0), (1, 0), (1, 1), (0, 0)]
    with pytest.raises(TypeError, match=r"\(n, 2\) array"):
        regions.simplify_contour(LinearRing(), 1.0)
    with pytest.raises(TypeError, match=r"\(n, 2\) array"):
        regions.simplify_contours([LinearRing()], 1.0)


def test_graph_simplify_takes_a_batched_simplifier():
    """MorphologicalGraph.simplify hands all its curves to the function it is given, once, after the merges; without
    one it is what it was"""
    from video.analysis import curves
    from video.analysis.morphological_graph import MorphologicalGraph

    def graph():
        g = MorphologicalGraph()
        for k, xy in enumerate([(0, 0), (10, 0), (20, 0), (20, 10)], 1):
            g.add_node(k, coords=xy)
        g.add_edge_line(1, 2, np.array([[0, 0], [3, 0], [6, 1], [10, 0]]))
        g.add_edge_line(2, 3, np.array([[10, 0], [15, 0], [20, 0]]))
        g.add_edge_line(3, 4, np.array([[20, 0], [20, 5], [21, 7], [20, 10]]))
        return g
    calls = []

    def batched(cs, eps):
        calls.append((len(cs), eps))
        return [curves.simplify_curve(c, eps) for c in cs]
    a, b, c = graph(), graph(), graph()
    a.simplify(0.5)
    b.simplify(0.5, simplify_curves=batched)
    c.merge_pass_through_nodes()
    assert calls == [(c.number_of_edges(), 0.5)] and a.number_of_edges() == b.number_of_edges() < 3
    for (_, _, da), (_, _, db), (_, _, dc) in zip(a.edges(data=True), b.edges(data=True), c.edges(data=True)):
        assert np.array_equal(da['curve'], db['curve']) and da['length'] == db['length']
        assert np.array_equal(da['curve'], curves.simplify_curve(dc['curve'], 0.5))
