"""GPU: geodesic distance maps, the shortest-path walk and the farthest-point iteration
(va_geodesic.hip, va_contours.hip) bit-exact against the restatements of tests/golden/make_golden_geodesic.py,
the committed fixture, scipy's Dijkstra and the oracle's cv2.findContours restatement."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_geodesic", os.path.join(ROOT, "tests", "golden", "make_golden_geodesic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()


@pytest.fixture(scope="module")
def geo():
    from video import _hip
    _hip.lib()
    return np.load(os.path.join(ROOT, "tests", "golden", "geodesic_v1.npz"), allow_pickle=False)


def arc_length(contour):
    """cv2.arcLength(contour, closed=True): float32 differences and sqrt, summed in double from the
    closing segment on"""
    pts = np.asarray(contour).reshape(-1, 2).astype(np.float32)
    per, prev = 0.0, pts[-1]
    for p in pts:
        d = p - prev
        per += float(np.sqrt(np.float32(d[0] * d[0] + d[1] * d[1])))
        prev = p
    return per


def default_p1(mask, oracle):
    contours = oracle.find_contours_external_simple(mask)
    c = max(contours, key=arc_length)
    return int(c[0, 0, 0]), int(c[0, 0, 1])


def test_fixture_maps_paths_and_farthest_points(geo):
    from video.analysis import regions
    for name in geo["names"]:
        mask = geo[name + "/mask"]
        starts = [tuple(p) for p in geo[name + "/starts"]]
        e = geo[name + "/ends"]
        ends = [tuple(p) for p in e] if len(e) else None
        for dt in (np.int64, np.int32):
            m = mask.astype(dt)
            assert regions.make_distance_map(m, starts, ends) is None
            assert m.dtype == dt and np.array_equal(m, geo[name + "/map"]), name
        end = tuple(int(v) for v in geo[name + "/path_end"])
        if end != (-1, -1):
            assert np.array_equal(regions.shortest_path_in_distance_map(geo[name + "/map"], end),
                                  geo[name + "/path"]), name
        fg = (mask != 0).astype(np.uint8)
        if fg.any():
            p1 = tuple(int(v) for v in geo[name + "/fp_p1_in"])
            a, b = regions.get_farthest_points(fg, p1)
            assert np.array_equal(np.array([a, b]), geo[name + "/fp"]), name
            assert np.array_equal(regions.get_farthest_points(fg, p1, ret_path=True), geo[name + "/fp_path"]), name


def test_random_masks_against_the_restatement():
    from video.analysis import regions
    rng = np.random.default_rng(5)
    for k in range(6):
        h, w = int(rng.integers(20, 130)), int(rng.integers(20, 170))
        mask = G.blobs(rng, h, w, frac=float(rng.uniform(0.4, 0.75)))
        ys, xs = np.nonzero(mask)
        starts = [(int(xs[i]), int(ys[i])) for i in rng.integers(0, len(xs), 1 + k % 3)]
        m = mask.copy()
        regions.make_distance_map(m, starts)
        ref = G.distance_map(mask, starts)
        assert np.array_equal(m, ref), k
        y, x = np.unravel_index(ref.argmax(), ref.shape)
        assert np.array_equal(regions.shortest_path_in_distance_map(ref, (x, y)), G.shortest_path(ref, (x, y)))
        fg = mask.astype(np.uint8)
        p1 = (int(xs[0]), int(ys[0]))
        assert regions.get_farthest_points(fg, p1) == G.farthest_points(fg, p1)
        assert np.array_equal(regions.get_farthest_points(fg, p1, ret_path=True),
                              G.farthest_points(fg, p1, ret_path=True))


def _snake(h, w, corridor=3, wall=3):
    m = np.zeros((h, w), np.int64)
    y, k = 0, 0
    while y + corridor <= h:
        m[y:y + corridor, :] = 1
        if y + corridor + wall + corridor <= h:   # the turn to the next corridor, alternating sides
            xs = slice(w - corridor, w) if k % 2 == 0 else slice(0, corridor)
            m[y + corridor:y + corridor + wall, xs] = 1
        y += corridor + wall
        k += 1
    return m


def test_1080p_snake_against_csgraph():
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra
    from video import ops
    h, w = 1080, 1920
    m = _snake(h, w)
    fill = m == 1
    out = ops.distance_map(fill, [(0, 0)])
    ys, xs = np.nonzero(fill)
    idx = -np.ones((h, w), np.int64)
    idx[ys, xs] = np.arange(len(ys))
    rows, cols, wts = [], [], []
    for dy, dx, c in ((0, 1, 1.0), (1, 0, 1.0), (1, 1, np.sqrt(2)), (1, -1, np.sqrt(2))):
        ny, nx = ys + dy, xs + dx
        ok = (ny < h) & (nx >= 0) & (nx < w)
        ok[ok] &= fill[ny[ok], nx[ok]]
        rows.append(idx[ys[ok], xs[ok]])
        cols.append(idx[ny[ok], nx[ok]])
        wts.append(np.full(ok.sum(), c))
    g = coo_matrix((np.concatenate(wts), (np.concatenate(rows), np.concatenate(cols))),
                   shape=(len(ys),) * 2).tocsr()
    d = dijkstra(g, directed=False, indices=0)
    assert np.isfinite(d).all() and d.max() > 1e4          # geodesics of more than 10^4 steps
    expect = np.floor(2 + d).astype(np.int64)
    got = out[ys, xs].astype(np.int64)
    near = np.abs(d - np.round(d)) < 1e-6                   # float sums at an integer: either side
    assert np.array_equal(got[~near], expect[~near])
    assert (np.abs(got[near] - (2 + np.round(d[near]))) <= 1).all()
    assert (out[~fill] == 0).all()


def test_batch_equals_per_frame_calls(oracle):
    from video import ops
    rng = np.random.default_rng(11)
    h, w = 72, 96
    frames = np.stack([G.blobs(rng, h, w, frac=0.5).astype(np.uint8) for _ in range(5)])
    frames[2] = 0                                           # an empty frame
    p1s = np.array([[3, 4], [50, 30], [7, 7], [-4, 9], [95, 71]])
    a, b = ops.farthest_points(frames, p1s)
    paths = ops.farthest_points(frames, p1s, ret_path=True)
    da, db = ops.farthest_points(frames)
    dpaths = ops.farthest_points(frames, ret_path=True)
    for f in range(len(frames)):
        sa, sb = ops.farthest_points(frames[f], tuple(p1s[f]))
        assert np.array_equal(a[f], sa) and np.array_equal(b[f], sb), f
        assert np.array_equal(paths[f], ops.farthest_points(frames[f], tuple(p1s[f]), ret_path=True)), f
        if frames[f].any():
            assert ((int(sa[0]), int(sa[1])), (int(sb[0]), int(sb[1]))) == \
                G.farthest_points(frames[f], tuple(int(v) for v in p1s[f]))
            ea, eb = ops.farthest_points(frames[f])
            assert np.array_equal(da[f], ea) and np.array_equal(db[f], eb), f
            assert np.array_equal(dpaths[f], ops.farthest_points(frames[f], ret_path=True)), f
            assert ((int(ea[0]), int(ea[1])), (int(eb[0]), int(eb[1]))) == \
                G.farthest_points(frames[f], default_p1(frames[f], oracle))
        else:
            assert tuple(da[f]) == (-1, -1) and len(dpaths[f]) == 0
    maps = ops.distance_map(frames, [[(3, 4)], [], [(0, 0)], [(-4, 9), (60, 40)], [(95, 71), (1, 1)]])
    single = [ops.distance_map(frames[f], l) for f, l in
              enumerate([[(3, 4)], [], [(0, 0)], [(-4, 9), (60, 40)], [(95, 71), (1, 1)]])]
    assert np.array_equal(maps, np.stack(single))


def _ring_with_wiggly_blob(h=120, w=120):
    m = np.zeros((h, w), np.uint8)
    m[10:110, 10:110] = 1
    m[12:108, 12:108] = 0                                   # a thin ring: perimeter ~ 2 * 4 * 99
    for y in range(20, 100, 4):                             # a comb inside: a much longer outline
        m[y:y + 2, 20:100] = 1
    m[20:100, 20:22] = 1
    return m


def test_default_p1_is_the_longest_external_contour(oracle):
    from video.analysis import regions
    m = _ring_with_wiggly_blob()
    contours = oracle.find_contours_external_simple(m)
    assert len(contours) == 1                               # the comb is nested: not external
    lengths = [arc_length(c) for c in contours]
    p1 = default_p1(m, oracle)
    assert regions.get_farthest_points(m) == G.farthest_points(m, p1)
    # the same comb outside the ring beats it
    big = np.zeros((120, 260), np.uint8)
    big[:, :120] = m
    big[20:100, 150:152] = 1
    for y in range(20, 100, 4):
        big[y:y + 2, 150:230] = 1
    contours = oracle.find_contours_external_simple(big)
    lengths = [arc_length(c) for c in contours]
    assert len(contours) == 2 and max(lengths) > min(lengths)
    p1 = default_p1(big, oracle)
    assert p1[0] >= 150
    assert regions.get_farthest_points(big) == G.farthest_points(big, p1)


def test_default_p1_ties_and_empty_masks(oracle):
    from video.analysis import regions
    m = np.zeros((40, 60), np.uint8)
    m[5:15, 5:15] = 1                                       # three squares of equal perimeter
    m[5:15, 30:40] = 1
    m[25:35, 10:20] = 1
    p1 = default_p1(m, oracle)
    assert p1 == (10, 25)                                   # the last first pixel in raster order
    assert regions.get_farthest_points(m) == G.farthest_points(m, p1)
    with pytest.raises(ValueError):
        regions.get_farthest_points(np.zeros((10, 10), np.uint8))
    with pytest.raises(ValueError):
        regions.get_farthest_points(np.zeros((10, 10), np.uint8), ret_path=True)


def test_p1_outside_the_mask():
    from video.analysis import regions
    rng = np.random.default_rng(3)
    m = G.blobs(rng, 50, 70).astype(np.uint8)
    ys, xs = np.nonzero(m == 0)
    for p1 in ((-3, 5), (500, 2), (-1, -1), (-3, -5), (2 ** 40, 2 ** 40), (int(xs[0]), int(ys[0]))):
        assert regions.get_farthest_points(m, p1) == G.farthest_points(m, p1), p1
        assert np.array_equal(regions.get_farthest_points(m, p1, ret_path=True),
                              G.farthest_points(m, p1, ret_path=True)), p1
    small = np.zeros((10, 10), np.uint8)
    small[3:7, 2:8] = 1
    for p1 in ((-1, -1), (-3, -5)):
        assert regions.get_farthest_points(small, p1) == G.farthest_points(small, p1) == ((7, 6), (2, 3))
    # an empty mask: the loop stops at once and hands the given start back unchanged
    empty = np.zeros((6, 7), np.uint8)
    for p1 in ((-1, -1), (2, 3), (2 ** 40, -7)):
        assert regions.get_farthest_points(empty, p1) == G.farthest_points(empty, p1) == (p1, (0, 0))


def test_outside_start_through_the_c_abi():
    """(-1, -1) is an ordinary start for the caller: ignored by the map, never 'no component'"""
    from video import ops
    small = np.zeros((2, 10, 10), np.uint8)
    small[:, 3:7, 2:8] = 1
    a, b = ops.farthest_points(small, np.array([[-1, -1], [-3, -5]]))
    assert a.tolist() == [[7, 6], [7, 6]] and b.tolist() == [[2, 3], [2, 3]]


def test_path_end_on_a_wall_raises():
    from video.analysis import regions
    d = np.zeros((5, 5), np.int64)
    d[2, 1:4] = [2, 3, 4]
    with pytest.raises(ValueError):
        regions.shortest_path_in_distance_map(d, (0, 0))
    assert regions.shortest_path_in_distance_map(d, (3, 2)).tolist() == [[3, 2], [2, 2], [1, 2]]


def test_two_shapes_back_to_back_on_a_created_stream():
    from video import _hip
    from video._hip import DeviceBuffer, check
    L = _hip.lib()
    stream = C.c_void_p()
    check(L.va_stream_create(C.byref(stream)))
    rng = np.random.default_rng(9)
    try:
        for (n, h, w) in ((3, 90, 130), (2, 41, 300), (3, 90, 130)):
            masks = np.stack([G.blobs(rng, h, w).astype(np.uint8) for _ in range(n)])
            p1 = np.array([[int(np.nonzero(f)[1][0]), int(np.nonzero(f)[0][0])] for f in masks], np.int32)
            wsb = L.va_geodesic_workspace_bytes(n, h, w)
            src, pin, ws = DeviceBuffer.from_array(masks), DeviceBuffer.from_array(p1), DeviceBuffer(wsb)
            p1o, p2o, dist, rounds = DeviceBuffer(n * 8), DeviceBuffer(n * 8), DeviceBuffer(n * 4), DeviceBuffer(n * 8)
            cap = 4096
            path, npath = DeviceBuffer(n * cap * 8), DeviceBuffer(n * 4)
            check(L.va_farthest_points(src.ptr, n, h, w, pin.ptr, p1o.ptr, p2o.ptr, dist.ptr, rounds.ptr, path.ptr,
                                       cap, npath.ptr, ws.ptr, wsb, stream))
            check(L.va_stream_sync(stream))
            a, b = p1o.download((n, 2), np.int32), p2o.download((n, 2), np.int32)
            np_ = npath.download((n,), np.int32)
            pts = path.download((n, cap, 2), np.int32)
            for f in range(n):
                ea, eb = G.farthest_points(masks[f], tuple(int(v) for v in p1[f]))
                assert (tuple(a[f]), tuple(b[f])) == (ea, eb)
                assert np.array_equal(pts[f, :np_[f]], G.farthest_points(masks[f], tuple(int(v) for v in p1[f]),
                                                                         ret_path=True))
            assert (rounds.download((n, 2), np.int32)[:, 0] >= 2).all()
    finally:
        check(L.va_stream_destroy(stream))
