"""GPU: the outline queries (va_ray_hits, va_points_in_outlines, ops.ray_hits, ops.points_in_outlines and the public
functions of video.analysis.regions and video.analysis.shapes) against the NumPy restatement of the pinned
definition in tests/golden/make_golden_outline.py and the fixture outline_v1.npz.  Every float64 is compared as a
bit pattern, so -0.0 and the NaN pattern count; every case runs under 'lanes8' and 'lanes64' (and the rule of
implementation=None), which must agree byte for byte.  The library is loaded inside fixtures and tests only."""
import ctypes as C

import numpy as np
import pytest

from outline_checks import (G, bits, check_fixture_containment, check_fixture_rays, fixture_rings, load_fixture,
                            same_bits, same_results)

pytestmark = pytest.mark.gpu

IMPLS = ("lanes8", "lanes64", None)
NAN_BITS = np.uint64(0x7FF8000000000000)
SIZES = (1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 300)
CENTRE = np.array([50.0, 50.0])


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


@pytest.fixture(scope="module")
def ops():
    from video import _hip, ops
    _hip.lib()
    return ops


def _check_rays(ops, outlines, closed, a, f, index, want=None, what=None, **kw):
    if want is None:
        want = G.ray_hits(outlines, closed, a, f, np.arange(len(outlines)) if index is None and len(outlines) > 1
                          else np.zeros(len(a), int) if index is None else index)
    first = None
    for impl in IMPLS:
        got = ops.ray_hits(outlines, closed, a, f, index, implementation=impl, **kw)
        same_results(got, want, (what, impl))
        raw = b"".join(np.ascontiguousarray(g).tobytes() for g in got)
        first = raw if first is None else first
        assert raw == first, (what, impl)
    return want


def _check_inside(ops, rings, p, index, want=None, what=None, **kw):
    if want is None:
        want = G.contains_points(rings, p, np.zeros(len(p), int) if index is None else index)
    for impl in IMPLS:
        got = ops.points_in_outlines(rings, p, index, implementation=impl, **kw)
        assert got.dtype == np.bool_ and np.array_equal(got, want), (what, impl)
    return want


def _rays(rng, count, grid):
    """count rays from inside a star ring about CENTRE and count from outside it, towards its middle and beyond"""
    ang = rng.uniform(0, 2 * np.pi, count)
    a_in = CENTRE + rng.uniform(-3, 3, (count, 2))
    f_in = a_in + 1000 * np.stack([np.cos(ang), np.sin(ang)], 1)
    ang = rng.uniform(0, 2 * np.pi, count)
    a_out = CENTRE + rng.uniform(60, 90, (count, 1)) * np.stack([np.cos(ang), np.sin(ang)], 1)
    f_out = a_out + 2.5 * (CENTRE + rng.uniform(-10, 10, (count, 2)) - a_out)
    a, f = np.concatenate([a_in, a_out]), np.concatenate([f_in, f_out])
    return (np.round(a * 2) / 2, np.round(f * 2) / 2) if grid else (a, f)


@pytest.fixture(scope="module")
def boundary():
    """the rings at the group boundaries, each closed and open, on the half-integer grid and off it, an outline of
    no points and one of one point, 16 rays from inside and 16 from outside each, and the restated results --
    computed once and left unchanged"""
    rng = np.random.default_rng(77)
    names, outlines, closed, a, f, index = [], [], [], [], [], []
    for n in SIZES:
        for is_closed in (True, False):
            for grid in (True, False):
                names.append("n%d_%s_%s" % (n, "closed" if is_closed else "open", "grid" if grid else "free"))
                outlines.append(G.star_ring(rng, n, step=0.5 if grid else None))
                closed.append(is_closed)
                ra, rf = _rays(rng, 16, grid)
                a.append(ra), f.append(rf), index.append(np.full(32, len(outlines) - 1))
    for name, pts in (("no_points", np.zeros((0, 2))), ("one_point", np.array([[50.0, 50.0]]))):
        names.append(name), outlines.append(pts), closed.append(True)
        ra, rf = _rays(rng, 16, True)
        a.append(ra), f.append(rf), index.append(np.full(32, len(outlines) - 1))
    a, f, index = np.concatenate(a), np.concatenate(f), np.concatenate(index)
    want = G.ray_hits(outlines, closed, a, f, index)
    assert 0.4 < np.mean(want[2] >= 0) < 0.98                  # hits and misses
    assert np.all(want[3][index >= len(SIZES) * 4] == 0)       # no points, one point: no hit, count 0
    cp, cindex = [], []
    for k, pts in enumerate(outlines):
        if len(pts):
            p = G.contain_points(names[k], pts)
            cp.append(p), cindex.append(np.full(len(p), k))
    cp, cindex = np.concatenate(cp), np.concatenate(cindex)
    inside = G.contains_points(outlines, cp, cindex)
    assert inside.any() and not inside.all()
    return dict(names=names, outlines=outlines, closed=closed, a=a, f=f, index=index, want=want, cp=cp,
                cindex=cindex, inside=inside)


# ------------------------------------------------------------------------------------------------ fixture
@pytest.mark.parametrize("crossover", [None, 0, 2 ** 31], ids=["rule", "all_lanes64", "all_lanes8"])
def test_public_functions_reproduce_the_fixture(ops, fx, monkeypatch, crossover):
    """every ray/*, fan/* and contains/* entry through the public functions, the NaN and inf anchors included;
    the public functions take no implementation, so the crossover of the rule is moved to either end"""
    if crossover is not None:
        monkeypatch.setattr(ops, "OUTLINE_WIDE_MIN_EDGES", crossover)
    assert any(np.isnan(c[1][0]) for c in G.RAY_CASES) and any(np.isinf(c[2][0]) for c in G.RAY_CASES)
    check_fixture_rays(fx)
    check_fixture_containment(fx)


def test_all_fixture_rays_as_one_batch(ops, fx):
    outs = G.outlines()
    names = sorted(outs)
    assert len(names) == 28 and len(G.RAY_CASES) == 30
    outlines, closed = [outs[n][0] for n in names], [outs[n][1] for n in names]
    a, f = np.array([c[1] for c in G.RAY_CASES]), np.array([c[2] for c in G.RAY_CASES])
    index = np.array([names.index(c[0]) for c in G.RAY_CASES])
    want = _check_rays(ops, outlines, closed, a, f, index)
    for k in range(30):
        assert np.array_equal(bits(want[1][k]), bits(fx["ray/%d/hit" % k])), k
    rings = fixture_rings(fx)
    order = sorted(rings)
    p = np.concatenate([rings[n][1] for n in order])
    pidx = np.repeat(np.arange(len(order)), [len(rings[n][1]) for n in order])
    _check_inside(ops, [rings[n][0] for n in order], p, pidx, want=np.concatenate([rings[n][2] for n in order]))


# -------------------------------------------------------------------------------------------- signed zeros
def test_a_quotient_that_underflows_to_minus_zero_hits(ops):
    outline, a, f = [np.array([(-1e-300, -1.0), (-1e-300, 1.0)])], [(0.0, 0.0)], [(1e100, 0.0)]
    want = _check_rays(ops, outline, [False], a, f, None)
    t, hits, edge, count = ops.ray_hits(outline, [False], a, f)
    assert bits(t)[0] == bits(-0.0) and np.signbit(want[0][0])
    assert hits.tolist() == [[0.0, 0.0]] and not np.signbit(hits).any()
    assert edge.tolist() == [0] and count.tolist() == [1]


def test_plus_and_minus_zero_tie_and_the_lower_edge_wins(ops):
    square, a, f = [np.array(G.SQUARE)], [(1.0, 0.0)], [(-1.0, 2.0)]
    te, hit = G.ray_edges(a[0], f[0], square[0], True)
    assert hit.all() and bits(te[0]) == bits(0.0) and bits(te[1]) == bits(-0.0)
    _check_rays(ops, square, [True], a, f, None)
    for impl in IMPLS:
        t, hits, edge, count = ops.ray_hits(square, [True], a, f, implementation=impl)
        assert bits(t)[0] == bits(0.0) and edge.tolist() == [0] and count.tolist() == [4], impl
        assert hits.tolist() == [[1.0, 0.0]], impl


# ------------------------------------------------------------------------------- edge counts at the group boundaries
def test_boundary_batch_rays(ops, boundary):
    b = boundary
    _check_rays(ops, b["outlines"], b["closed"], b["a"], b["f"], b["index"], want=b["want"])


def test_boundary_outlines_each_alone(ops, boundary):
    b = boundary
    for k, name in enumerate(b["names"]):
        pick = b["index"] == k
        want = tuple(w[pick] for w in b["want"])
        _check_rays(ops, [b["outlines"][k]], [b["closed"][k]], b["a"][pick], b["f"][pick], None, want=want, what=name)
        pick = b["cindex"] == k
        if pick.any():
            _check_inside(ops, [b["outlines"][k]], b["cp"][pick], None, want=b["inside"][pick], what=name)


def test_boundary_batch_containment(ops, boundary):
    b = boundary
    assert np.isnan(b["cp"]).any() and np.isinf(b["cp"]).any()
    _check_inside(ops, b["outlines"], b["cp"], b["cindex"], want=b["inside"])
    small = [k for k, o in enumerate(b["outlines"]) if len(o) < 3]
    assert len(small) >= 9
    p = np.full((len(small), 2), 50.0)
    assert not _check_inside(ops, b["outlines"], p, np.array(small)).any()


def test_one_long_outline(ops):
    rng = np.random.default_rng(5)
    ring = G.star_ring(rng, 5000)
    a, f = _rays(rng, 32, False)
    for is_closed in (True, False):
        want = _check_rays(ops, [ring], [is_closed], a, f, None)
        assert np.all(want[2][:32] >= 0) and want[2].max() > 64
    p = CENTRE + rng.uniform(-45, 45, (256, 2))
    p[:8] = ring[::700][:8]
    inside = _check_inside(ops, [ring], p, None)
    assert 20 < inside.sum() < 236


# --------------------------------------------------------------------------------------------------- ties
def test_ties(ops):
    rng = np.random.default_rng(9)
    outs = G.outlines()
    cases = [(outs[n][0], outs[n][1]) for n in ("box", "notch", "doubled", "unit_square", "unit_square_ring")]
    cases += [(G.star_ring(rng, n, step=1.0), c) for n, c in ((5, True), (12, True), (40, False), (70, True))]
    outlines, closed = [c[0] for c in cases], [c[1] for c in cases]
    a, f, index = [], [], []
    for k, (pts, is_closed) in enumerate(cases):
        mid = np.round(pts.mean(axis=0))
        nxt = np.roll(pts, -1, axis=0)
        rays = [(np.broadcast_to(mid, pts.shape), mid + 2 * (pts - mid)),      # through every vertex, t = 1/2
                (np.broadcast_to(mid, pts.shape), pts),                        # ending on every vertex, t = 1
                (pts - (nxt - pts), nxt + (nxt - pts)),                        # along every edge and beyond
                (pts, nxt),                                                    # exactly along every edge
                (pts, pts),                                                    # zero length, on a vertex
                (np.broadcast_to(mid, pts.shape), np.broadcast_to(mid, pts.shape))]
        for ra, rf in rays:
            a.append(ra), f.append(rf), index.append(np.full(len(ra), k))
    a, f, index = np.concatenate(a), np.concatenate(f), np.concatenate(index)
    want = G.ray_hits(outlines, closed, a, f, index)
    t, hits, edge, count = want
    assert np.sum(count >= 2) > 100                              # vertices reported by two edges, and more
    two = np.flatnonzero(count == 2)
    for k in two[:50]:                                           # a tie: the lower index is the answer
        te, hit = G.ray_edges(a[k], f[k], outlines[index[k]], closed[index[k]])
        assert edge[k] == np.flatnonzero(hit & (te == te[hit].min()))[0]
    assert np.any(count == 0)
    _check_rays(ops, outlines, closed, a, f, index, want=want)
    vertices = np.concatenate(outlines)
    vindex = np.repeat(np.arange(len(outlines)), [len(o) for o in outlines])
    assert not _check_inside(ops, outlines, vertices, vindex).any()


# ------------------------------------------------------------------------------------------------ envelope
def test_empty_calls(ops):
    from video import _hip
    L = _hip.lib()
    assert L.va_ray_hits(None, None, None, 0, 0, None, None, None, 0, 0, None, None, None, None, None) == 0
    assert L.va_points_in_outlines(None, None, 0, 0, None, None, 0, 64, None, None) == 0
    assert L.va_ray_hits(None, None, None, 0, 3, None, None, None, 0, 8, None, None, None, None, None) == 0
    # m == 0 with queries: nothing is enqueued, the outputs stay as they were
    out = _hip.DeviceBuffer.from_array(np.full(64, 0x11, np.uint8))
    assert L.va_ray_hits(None, None, None, 0, 0, None, None, None, 2, 0, out.ptr, out.ptr, out.ptr, out.ptr, None) == 0
    assert L.va_points_in_outlines(None, None, 0, 0, None, None, 2, 0, out.ptr, None) == 0
    assert np.all(out.download((64,), np.uint8) == 0x11)
    out.free()
    assert ops.ray_hits([np.array(G.SQUARE)], [True], [], [])[0].shape == (0,)
    assert ops.points_in_outlines([], []).shape == (0,)


def test_scrambled_index_and_odd_offsets(ops, boundary):
    b = boundary
    rng = np.random.default_rng(13)
    perm = rng.permutation(len(b["index"]))
    want = tuple(w[perm] for w in b["want"])
    _check_rays(ops, b["outlines"], b["closed"], b["a"][perm], b["f"][perm], b["index"][perm], want=want)
    perm = rng.permutation(len(b["cindex"]))
    _check_inside(ops, b["outlines"], b["cp"][perm], b["cindex"][perm], want=b["inside"][perm])
    # every outline after a one-point outline starts at an odd point offset
    pick = [b["names"].index(n) for n in ("n7_closed_free", "n64_open_grid", "n129_closed_free")]
    one = np.array([[50.0, 50.0]])
    outlines, closed, a, f, index, cp, cindex = [], [], [], [], [], [], []
    for k in pick:
        while sum(len(o) for o in outlines) % 2 == 0:
            outlines.append(one), closed.append(len(outlines) % 2 == 0)
        outlines.append(b["outlines"][k]), closed.append(b["closed"][k])
        slot = len(outlines) - 1
        assert sum(len(o) for o in outlines[:slot]) % 2 == 1
        sel = b["index"] == k
        a.append(b["a"][sel]), f.append(b["f"][sel]), index.append(np.full(sel.sum(), slot))
        sel = b["cindex"] == k
        cp.append(b["cp"][sel]), cindex.append(np.full(sel.sum(), slot))
    sel = np.isin(b["index"], pick)
    _check_rays(ops, outlines, closed, np.concatenate(a), np.concatenate(f), np.concatenate(index),
                want=tuple(w[sel] for w in b["want"]))
    _check_inside(ops, outlines, np.concatenate(cp), np.concatenate(cindex), want=b["inside"][np.isin(b["cindex"], pick)])


def test_more_queries_than_65535(ops):
    rng = np.random.default_rng(17)
    tri = np.array([(20.0, 20.0), (80.0, 30.0), (45.0, 85.0)])
    a, f = _rays(rng, 350, False)
    want = G.ray_hits([tri], [True], a, f, np.zeros(700, int))
    reps = 100
    _check_rays(ops, [tri], [True], np.tile(a, (reps, 1)), np.tile(f, (reps, 1)), None,
                want=(np.tile(want[0], reps), np.tile(want[1], (reps, 1)), np.tile(want[2], reps),
                      np.tile(want[3], reps)))
    p = CENTRE + rng.uniform(-40, 40, (700, 2))
    inside = G.contains_points([tri], p, np.zeros(700, int))
    assert 100 < inside.sum() < 600
    _check_inside(ops, [tri], np.tile(p, (reps, 1)), None, want=np.tile(inside, reps))


def test_more_outlines_than_65535(ops):
    rng = np.random.default_rng(19)
    tris = [G.star_ring(rng, 3) for _ in range(700)]
    a, f = _rays(rng, 350, False)
    p = CENTRE + rng.uniform(-30, 30, (700, 2))
    want = G.ray_hits(tris, [True] * 700, a, f, np.arange(700))
    inside = G.contains_points(tris, p, np.arange(700))
    reps = 100
    many = tris * reps
    assert len(many) == 70000
    _check_rays(ops, many, [True] * len(many), np.tile(a, (reps, 1)), np.tile(f, (reps, 1)), None,
                want=(np.tile(want[0], reps), np.tile(want[1], (reps, 1)), np.tile(want[2], reps),
                      np.tile(want[3], reps)))
    _check_inside(ops, many, np.tile(p, (reps, 1)), np.arange(len(many)), want=np.tile(inside, reps))


# ------------------------------------------------------------------------------------------------ refusals
class _Abi(object):
    """device copies of a batch for calls at the C ABI; the outputs start out as 0x11 bytes"""

    def __init__(self, outlines, closed, a, f, index, point_off=None):
        from video import _hip
        self.hip, self.L = _hip, _hip.lib()
        counts = [len(o) for o in outlines]
        self.m, self.q, self.npoints = len(outlines), len(index), int(sum(counts))
        off = np.cumsum([0] + counts).astype(np.int64) if point_off is None else np.asarray(point_off, np.int64)
        up = _hip.DeviceBuffer.from_array
        self.pts, self.off = up(np.concatenate(outlines).astype(np.float64)), up(off)
        self.closed = up(np.asarray(closed, np.uint8))
        self.a, self.f = up(np.asarray(a, np.float64)), up(np.asarray(f, np.float64))
        self.index = up(np.asarray(index, np.int32))
        self.out = [up(np.full(n * self.q, 0x11, np.uint8)) for n in (8, 16, 4, 4, 1)]

    def rays(self, lanes):
        t, h, e, c, _ = self.out
        rc = self.L.va_ray_hits(self.pts.ptr, self.off.ptr, self.closed.ptr, self.npoints, self.m, self.a.ptr,
                                self.f.ptr, self.index.ptr, self.q, lanes, t.ptr, h.ptr, e.ptr, c.ptr, None)
        assert rc == 0, self.L.va_last_error()
        return (t.download((self.q,), np.float64), h.download((self.q, 2), np.float64),
                e.download((self.q,), np.int32), c.download((self.q,), np.int32))

    def inside(self, lanes):
        rc = self.L.va_points_in_outlines(self.pts.ptr, self.off.ptr, self.npoints, self.m, self.a.ptr,
                                          self.index.ptr, self.q, lanes, self.out[4].ptr, None)
        assert rc == 0, self.L.va_last_error()
        return self.out[4].download((self.q,), np.uint8)

    def free(self):
        for buf in [self.pts, self.off, self.closed, self.a, self.f, self.index] + self.out:
            buf.free()


def test_refused_queries_leave_the_others_correct(boundary):
    b = boundary
    pick = [b["names"].index(n) for n in ("n9_closed_grid", "n65_open_free", "n300_closed_free")]
    outlines, closed = [b["outlines"][k] for k in pick], [b["closed"][k] for k in pick]
    sel = np.flatnonzero(np.isin(b["index"], pick))
    a, f = b["a"][sel], b["f"][sel]
    index = np.searchsorted(pick, b["index"][sel]).astype(np.int32)
    want = G.ray_hits(outlines, closed, a, f, index)
    inside = G.contains_points(outlines, a, index)
    bad = index.copy()
    bad[[0, 40, 95]] = (-1, 3, 2 ** 31 - 1)
    bad[[17, 50]] = (3, -7)
    refused = np.isin(np.arange(len(bad)), [0, 40, 95, 17, 50])
    abi = _Abi(outlines, closed, a, f, bad)
    try:
        for lanes in (8, 64, 0):
            t, hits, edge, count = abi.rays(lanes)
            assert np.all(bits(t[refused]) == NAN_BITS) and np.all(bits(hits[refused]) == NAN_BITS), lanes
            assert np.all(edge[refused] == -1) and np.all(count[refused] == -1), lanes
            same_results((t[~refused], hits[~refused], edge[~refused], count[~refused]),
                         tuple(w[~refused] for w in want), lanes)
            got = abi.inside(lanes)
            assert np.all(got[refused] == 2) and np.array_equal(got[~refused], inside[~refused].astype(np.uint8)), lanes
    finally:
        abi.free()
    # decreasing offsets, offsets beyond npoints and negative offsets refuse the outlines they bound, and only those
    counts = [len(o) for o in outlines]
    good = np.cumsum([0] + counts)
    for off, hurt in (([good[0], good[2], good[1], good[3]], {1}), ([good[0], good[1], good[2], good[3] + 1], {2}),
                      ([-1, good[1], good[2], good[3]], {0}), ([good[1], good[0], good[2], good[3]], {0})):
        abi = _Abi(outlines, closed, a, f, index, point_off=off)
        try:
            refused = np.isin(index, list(hurt))
            # an outline between two intact offsets may own other points than before: only its markers are checked
            moved = np.array([off[k] != good[k] or off[k + 1] != good[k + 1] for k in range(3)])[index]
            for lanes in (8, 64):
                t, hits, edge, count = abi.rays(lanes)
                assert np.all(count[refused] == -1) and np.all(edge[refused] == -1), (off, lanes)
                assert np.all(bits(t[refused]) == NAN_BITS) and np.all(bits(hits[refused]) == NAN_BITS)
                assert np.all(count[~refused] >= 0)
                same_results((t[~moved], hits[~moved], edge[~moved], count[~moved]), tuple(w[~moved] for w in want),
                             (off, lanes))
                got = abi.inside(lanes)
                assert np.all(got[refused] == 2) and np.all(got[~refused] <= 1)
                assert np.array_equal(got[~moved], inside[~moved].astype(np.uint8))
        finally:
            abi.free()


def test_invalid_arguments_at_the_abi_and_through_ops(ops):
    sq = np.array(G.SQUARE)
    abi = _Abi([sq], [True], [(0.5, 0.5)], [(2.0, 0.5)], [0])
    L, (t, h, e, c, s) = abi.L, abi.out
    try:
        for lanes in (1, 16, 32, -8, 128):
            assert L.va_ray_hits(abi.pts.ptr, abi.off.ptr, abi.closed.ptr, 4, 1, abi.a.ptr, abi.f.ptr, abi.index.ptr, 1,
                                 lanes, t.ptr, h.ptr, e.ptr, c.ptr, None) == -22
            assert b"va_ray_hits" in L.va_last_error() and b"lanes" in L.va_last_error()
            assert L.va_points_in_outlines(abi.pts.ptr, abi.off.ptr, 4, 1, abi.a.ptr, abi.index.ptr, 1, lanes, s.ptr,
                                           None) == -22
            assert b"va_points_in_outlines" in L.va_last_error() and b"lanes" in L.va_last_error()
        args = [abi.pts.ptr, abi.off.ptr, abi.closed.ptr, 4, 1, abi.a.ptr, abi.f.ptr, abi.index.ptr, 1, 8, t.ptr, h.ptr,
                e.ptr, c.ptr, None]
        for k in (0, 1, 2, 5, 6, 7, 10, 11, 12, 13):
            call = list(args)
            call[k] = None
            assert L.va_ray_hits(*call) == -22 and b"NULL" in L.va_last_error(), k
        args = [abi.pts.ptr, abi.off.ptr, 4, 1, abi.a.ptr, abi.index.ptr, 1, 64, s.ptr, None]
        for k in (0, 1, 4, 5, 8):
            call = list(args)
            call[k] = None
            assert L.va_points_in_outlines(*call) == -22 and b"NULL" in L.va_last_error(), k
        assert L.va_ray_hits(abi.pts.ptr, abi.off.ptr, abi.closed.ptr, -1, 1, abi.a.ptr, abi.f.ptr, abi.index.ptr, 1, 8,
                             t.ptr, h.ptr, e.ptr, c.ptr, None) == -22                  # a negative count
        assert np.all(t.download((8,), np.uint8) == 0x11)               # nothing was launched
    finally:
        abi.free()
    for index in ([-1], [1]):
        with pytest.raises(ValueError):
            ops.ray_hits([sq], [True], [(0.5, 0.5)], [(2.0, 0.5)], index=index)
        with pytest.raises(ValueError):
            ops.points_in_outlines([sq], [(0.5, 0.5)], index=index)
    with pytest.raises(ValueError):
        ops.ray_hits([np.zeros((3, 3))], [True], [(0.5, 0.5)], [(2.0, 0.5)])
    with pytest.raises(ValueError):
        ops.ray_hits([sq], [True], [(0.5, 0.5)], [(2.0, 0.5)], implementation="lanes32")


# -------------------------------------------------------------------------------------------- dirty memory
@pytest.mark.parametrize("fill", [0xFF, 0xA5], ids=["fill_ff", "fill_a5"])
def test_boundary_batch_on_dirty_memory(ops, boundary, fill):
    from video import _hip
    b = boundary
    ops.pool_clear()
    _hip.set_fill_mode(fill)
    try:
        assert _hip.lib().va_test_hook_fill(fill) == 0 and _hip.fill_mode() == fill
        for run in (1, 2):
            _check_rays(ops, b["outlines"], b["closed"], b["a"], b["f"], b["index"], want=b["want"], what=run)
            _check_inside(ops, b["outlines"], b["cp"], b["cindex"], want=b["inside"], what=run)
        found = _hip.check_guards()
    finally:
        _hip.set_fill_mode(-1)
        ops.pool_clear()
        _hip.check_guards()
    assert found == [], found


# ---------------------------------------------------------------------------------- determinism and stream
def test_two_runs_and_a_created_stream_give_the_same_bytes(ops, boundary):
    from video import _hip
    b = boundary
    L = _hip.lib()
    s = C.c_void_p()
    assert L.va_stream_create(C.byref(s)) == 0
    try:
        for impl in IMPLS:
            runs = [ops.ray_hits(b["outlines"], b["closed"], b["a"], b["f"], b["index"], implementation=impl, stream=st)
                    for st in (None, None, s.value)]
            for got in runs:
                same_results(got, b["want"], impl)
            ins = [ops.points_in_outlines(b["outlines"], b["cp"], b["cindex"], implementation=impl, stream=st)
                   for st in (None, None, s.value)]
            for got in ins:
                assert np.array_equal(got, b["inside"]), impl
    finally:
        assert L.va_stream_destroy(s) == 0


# -------------------------------------------------------------------------------------------------- wiring
def test_contours_of_find_contours_go_into_fans_and_containment(ops):
    from video.analysis import regions, shapes
    yy, xx = np.mgrid[:64, :80]
    stack = np.zeros((3, 64, 80), np.uint8)
    for k in range(3):
        for cx, cy, r in ((18 + 3 * k, 20, 9), (55, 40 - 4 * k, 12), (30, 50, 5 + k)):
            stack[k][(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = 255
        stack[k, 5:9, 60 + k:75] = 1
    contours = [c.reshape(-1, 2) for frame in ops.find_contours(stack) for c in frame]
    assert len(contours) >= 9 and all(c.dtype == np.int32 and len(c) >= 3 for c in contours)
    polys = [shapes.Polygon(c) for c in contours]
    anchors = [tuple(np.round(c.mean(axis=0) * 2) / 2) for c in contours]
    angles = [G.fan_angles(8 + k % 5, 0.1 * k) for k in range(len(contours))]
    fans = regions.ray_fans(polys, anchors, angles, ray_length=100)
    for k, (hits, dist) in enumerate(fans):
        points, _ = G.get_farthest_ray_intersection(anchors[k], angles[k], contours[k], True, 100)
        want = np.array([[np.nan, np.nan] if p is None else p for p in points], np.float64).reshape(-1, 2)
        same_bits(hits, want, k)
        same_bits(dist, np.array([G.point_distance(h, anchors[k]) for h in want], np.float64), k)
        assert np.isfinite(hits).all(), k
    cp = [G.contain_points("c%d" % k, c.astype(np.float64)) for k, c in enumerate(contours)]
    index = np.repeat(np.arange(len(cp)), [len(p) for p in cp])
    got = shapes.contains_points(polys, np.concatenate(cp), index)
    want = G.contains_points(contours, np.concatenate(cp), index)
    assert np.array_equal(got, want) and want.any() and not want.all()
