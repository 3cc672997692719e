"""CPU: the public layer of the outline queries (video.analysis.regions: get_ray_hitpoint, get_ray_intersections,
get_farthest_ray_intersection, ray_hits, ray_fans; video.analysis.shapes: Polygon.contains, Polygon.contains_points,
contains_points) with ops.ray_hits and ops.points_in_outlines replaced by adapters over the NumPy restatement: the
public layer alone reproduces the whole fixture outline_v1.npz, bit for bit.  Also the host-side ValueErrors of the
two ops, which are raised before a device is needed."""
import numpy as np
import pytest

from outline_checks import (G, Coords, bits, check_fixture_containment, check_fixture_rays, load_fixture,
                            outline_forms, same_bits)


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


@pytest.fixture
def restated(monkeypatch):
    """the two ops as the restatement, with the ops' own argument conventions; counts the calls"""
    from video import ops
    calls = {"ray_hits": 0, "points_in_outlines": 0, "rays": 0}

    def index_of(index, m, q):
        if index is None:
            return np.zeros(q, np.int64) if m == 1 else np.arange(m)
        return np.asarray(index, np.int64)

    def ray_hits(outlines, closed, anchors, fars, index=None, implementation=None, stream=None):
        a, f = np.asarray(anchors, np.float64).reshape(-1, 2), np.asarray(fars, np.float64).reshape(-1, 2)
        calls["ray_hits"] += 1
        calls["rays"] += len(a)
        assert len(a) > 0, "an empty batch must not reach the op"
        t, hits, edge, count = G.ray_hits(outlines, closed, a, f, index_of(index, len(outlines), len(a)))
        return t, hits, edge, count

    def points_in_outlines(outlines, points, index=None, implementation=None, stream=None):
        p = np.asarray(points, np.float64).reshape(-1, 2)
        calls["points_in_outlines"] += 1
        return G.contains_points(outlines, p, index_of(index, len(outlines), len(p)))

    monkeypatch.setattr(ops, "ray_hits", ray_hits)
    monkeypatch.setattr(ops, "points_in_outlines", points_in_outlines)
    return calls


def test_public_ray_functions_reproduce_the_fixture(fx, restated):
    made = check_fixture_rays(fx)
    # one op call per public call, except the fans without angles: those make none
    outs = G.outlines()
    empty = sum(2 * len(outline_forms(*outs[case[0]])[:2]) for case in G.FAN_CASES if case[2] == 0)
    assert empty > 0 and restated["ray_hits"] == made - empty


def test_public_containment_reproduces_the_fixture(fx, restated):
    check_fixture_containment(fx)
    assert restated["points_in_outlines"] > 20


def test_argument_forms_agree(restated):
    from video.analysis import regions
    from video.analysis.shapes import Polygon
    square = np.array(G.SQUARE)
    ring = np.concatenate([square, square[:1]])
    want = ((1.0, 0.5), 0.5)
    assert regions.get_ray_hitpoint((0.5, 0.5), (2.0, 0.5), Polygon(square), ret_dist=True) == want
    assert regions.get_ray_hitpoint((0.5, 0.5), (2.0, 0.5), ring, ret_dist=True) == want
    assert regions.get_ray_hitpoint((0.5, 0.5), (2.0, 0.5), ring.tolist(), ret_dist=True) == want
    assert regions.get_ray_hitpoint((0.5, 0.5), (2.0, 0.5), Coords(ring), ret_dist=True) == want
    # an (N, 2) array is open as given: the four points alone have no edge towards x = -1; the Polygon has
    assert regions.get_ray_hitpoint((0.5, 0.5), (-1.0, 0.5), square) is None
    none, dist = regions.get_ray_hitpoint((0.5, 0.5), (-1.0, 0.5), Coords(square), ret_dist=True)
    assert none is None and isinstance(dist, float) and np.isnan(dist)
    assert regions.get_ray_hitpoint((0.5, 0.5), (-1.0, 0.5), Polygon(square)) == (0.0, 0.5)


def test_a_fan_is_one_call_and_no_angles_make_none(restated):
    from video.analysis import regions
    from video.analysis.shapes import Polygon
    poly = Polygon(np.array(G.SQUARE))
    angles = G.fan_angles(8, 0.0)
    points = regions.get_ray_intersections((0.5, 0.5), angles, poly)
    assert restated["ray_hits"] == 1 and restated["rays"] == 8 and len(points) == 8
    regions.get_farthest_ray_intersection((0.5, 0.5), angles, poly)
    assert restated["ray_hits"] == 2 and restated["rays"] == 16
    assert regions.get_ray_intersections((0.5, 0.5), [], poly) == []
    assert regions.get_farthest_ray_intersection((0.5, 0.5), np.zeros(0), poly) == (None, 0, None)
    assert restated["ray_hits"] == 2
    regions.get_ray_hitpoint((0.5, 0.5), (2.0, 0.5), poly)
    assert restated["ray_hits"] == 3 and restated["rays"] == 17


def test_farthest_keeps_the_first_of_equal_maxima_and_needs_a_strict_maximum(restated):
    from video.analysis import regions
    from video.analysis.shapes import Polygon
    poly = Polygon(np.array(G.SQUARE))
    # the four axis rays from the centre all hit at distance 0.5: the first angle stays
    angles = [0.0, np.pi, 0.0]
    want_points, want = G.get_farthest_ray_intersection((0.5, 0.5), angles, G.SQUARE, True)
    got = regions.get_farthest_ray_intersection((0.5, 0.5), angles, poly)
    assert got[1] == 0.5 and got[2] == 0.0 and got[2] is angles[0] and got == want
    # a strictly larger distance replaces it, an equal one later does not
    angles = [0.0, np.pi / 4, 0.0, np.pi / 4]
    got = regions.get_farthest_ray_intersection((0.5, 0.5), angles, poly)
    assert got == G.get_farthest_ray_intersection((0.5, 0.5), angles, G.SQUARE, True)[1]
    assert got[2] is angles[1] and got[1] > 0.5
    # nothing hit: the start value, distance 0 as an int
    far_away = regions.get_farthest_ray_intersection((5.0, 5.0), [0.0, 1.0], poly, ray_length=1)
    assert far_away == (None, 0, None) and type(far_away[1]) is int
    assert regions.get_ray_intersections((5.0, 5.0), [0.0, 1.0], poly, ray_length=1) == [None, None]


def test_batched_forms_equal_the_single_calls(fx, restated):
    from video.analysis import regions
    from video.analysis.shapes import Polygon
    outs = G.outlines()
    cases = [c for c in G.FAN_CASES]
    shapes_ = [Polygon(outs[c[0]][0]) if outs[c[0]][1] else outs[c[0]][0] for c in cases]
    anchors = [c[1] for c in cases]
    angles = [fx["fan/%d/angles" % k] for k in range(len(cases))]
    lengths = sorted({c[4] for c in cases})
    before = restated["ray_hits"]
    for length in lengths:
        pick = [k for k, c in enumerate(cases) if c[4] == length]
        fans = regions.ray_fans([shapes_[k] for k in pick], [anchors[k] for k in pick], [angles[k] for k in pick],
                                length)
        assert len(fans) == len(pick)
        for k, (hits, dist) in zip(pick, fans):
            same_bits(hits, fx["fan/%d/hits" % k], k)
            want = np.array([G.point_distance(h, anchors[k]) for h in hits], np.float64).reshape(-1)
            same_bits(dist, want, k)
    assert restated["ray_hits"] == before + len(lengths)          # one launch per ray_fans call
    assert regions.ray_fans([], [], []) == []
    none = regions.ray_fans([shapes_[0]], [(0.5, 0.5)], [[]])
    assert len(none) == 1 and none[0][0].shape == (0, 2) and none[0][1].shape == (0,)
    assert restated["ray_hits"] == before + len(lengths)
    with pytest.raises(ValueError):
        regions.ray_fans([shapes_[0]], [(0.5, 0.5)], [])
    # ray_hits: all single rays of the fixture as one batch
    names = sorted(outs)
    forms = [Polygon(outs[n][0]) if outs[n][1] else outs[n][0] for n in names]
    a = np.array([c[1] for c in G.RAY_CASES])
    f = np.array([c[2] for c in G.RAY_CASES])
    index = np.array([names.index(c[0]) for c in G.RAY_CASES])
    hits, dist, edge = regions.ray_hits(forms, a, f, index)
    assert edge.dtype == np.int32 and hits.shape == (30, 2)
    for k in range(len(G.RAY_CASES)):
        assert np.array_equal(bits(hits[k]), bits(fx["ray/%d/hit" % k])), k
        assert np.array_equal(bits(dist[k]), bits(fx["ray/%d/dist" % k])), k
        assert (edge[k] < 0) == bool(np.isnan(fx["ray/%d/hit" % k]).any()), k


def test_ops_raise_on_the_host_before_a_device_is_needed():
    """(no monkeypatch: the real ops; every one of these is refused before the library is asked for a GPU)"""
    from video import ops
    sq = np.array(G.SQUARE)
    a, f = [(0.5, 0.5)], [(2.0, 0.5)]
    for index in ([-1], [1], [0, 0]):
        with pytest.raises(ValueError):
            ops.ray_hits([sq], [True], a, f, index=index)
        with pytest.raises(ValueError):
            ops.points_in_outlines([sq], a, index=index)
    with pytest.raises(ValueError):
        ops.ray_hits([sq, sq], [True, True], a, f)                      # no index: one ray per outline
    with pytest.raises(ValueError):
        ops.points_in_outlines([sq, sq, sq], [(0.5, 0.5), (0.2, 0.2)])
    with pytest.raises(ValueError):
        ops.ray_hits([], [], a, f)                                      # no outline to name
    for bad in (np.zeros((4, 3)), np.zeros(4), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            ops.ray_hits([sq, bad], [True, True], a * 2, f * 2)
        with pytest.raises(ValueError):
            ops.points_in_outlines([bad], a)
    with pytest.raises(ValueError):
        ops.ray_hits([sq], [True, False], a, f)                         # one flag per outline
    with pytest.raises(ValueError):
        ops.ray_hits([sq], [True], a, f * 2)                            # as many far points as anchors
    with pytest.raises(ValueError):
        ops.ray_hits([sq], [True], [(0.5, 0.5, 0.5)], f)
    for name in ("lanes16", "auto", 8):
        with pytest.raises(ValueError):
            ops.ray_hits([sq], [True], a, f, implementation=name)
        with pytest.raises(ValueError):
            ops.points_in_outlines([sq], a, implementation=name)
    # empty query lists: empty arrays, no device
    t, hits, edge, count = ops.ray_hits([sq], [True], np.zeros((0, 2)), [])
    assert (t.shape, hits.shape, edge.shape, count.shape) == ((0,), (0, 2), (0,), (0,))
    assert (t.dtype, hits.dtype, edge.dtype, count.dtype) == (np.float64, np.float64, np.int32, np.int32)
    inside = ops.points_in_outlines([sq], [])
    assert inside.shape == (0,) and inside.dtype == np.bool_
    assert ops.points_in_outlines([], []).shape == (0,)
    assert ops.ray_hits([], [], [], [])[1].shape == (0, 2)
