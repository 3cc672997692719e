"""CPU: the contour fixture (tests/golden/contours_v1.npz), the oracle's Suzuki-Abe scanner against the
topological definition the GPU path uses (tests/golden/make_golden_contours.py: topological_starts), and the host
side of find_contours / get_external_contour.  Needs no GPU and no reference checkout."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_contours", os.path.join(ROOT, "tests", "golden", "make_golden_contours.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(ROOT, "tests", "golden", "contours_v1.npz"), allow_pickle=False)


def test_fixture_is_complete_and_the_oracle_reproduces_it(fx, oracle):
    assert len(fx["shims"]) == 5
    cases = G.all_cases()
    assert len(cases) == len(G.WIDTHS) * len(G.HEIGHTS) * len(G.DENSITIES) + 4 + 10 + 9 + 3
    for name, mask in cases.items():
        pts, sizes = G.flatten(oracle.find_contours_external_simple(mask))
        assert np.array_equal(pts, fx["c/%s/points" % name]), name
        assert np.array_equal(sizes, fx["c/%s/sizes" % name]), name
    for name, (mask, sizes) in G.fixed_cases().items():
        assert list(fx["c/fixed/%s/sizes" % name]) == sizes, name
    for key, ring, res in G.ring_cases():
        assert np.array_equal(fx[key + "/points"], ring), key
        assert fx[key].ndim == 2 and fx[key].shape[1] == 2 and len(fx[key]) > 2, key
        assert np.isnan(fx[key + "/resolution"]) if res is None else float(fx[key + "/resolution"]) == res, key
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "contours_v1.npz")) < 200 * 1024


def test_topological_rule_equals_the_oracle(oracle):
    """first raster pixels of the 8-connected components that lie in no hole, by descending index == the start
    points of the oracle's contours, in its order; every contour starts at its component's first pixel"""
    nested = total = 0
    masks = list(G.all_cases().values()) + list(G.seeded_check_masks())
    for k, mask in enumerate(masks):
        contours = oracle.find_contours_external_simple(mask)
        starts, ncomp = G.topological_starts(mask)
        ref = np.array([c[0, 0] for c in contours], np.int64).reshape(-1, 2)
        assert np.array_equal(starts, ref), k
        nested += ncomp > len(contours)
        total += 1
    assert total >= 400 and nested >= 50


def test_find_contours_argument_checks_need_no_device():
    from video import ops
    for bad in (np.zeros(5, np.uint8), np.zeros((2, 2, 3, 3), np.uint8)):
        with pytest.raises(ValueError):
            ops.find_contours(bad)
    assert ops.find_contours(np.zeros((0, 5, 7), np.uint8)) == []
    assert ops.find_contours(np.zeros((0, 5, 7), np.uint8), ret_info=True, moments=True) == ([], [], [])
    from video.analysis import regions
    assert regions.find_contours(np.zeros((0, 5, 7), np.uint8)) == []
    assert regions.get_external_contours([]) == []


def test_external_contour_resolution_rule():
    from video.analysis.regions import external_contour_resolution as res
    # half the smallest non-zero distance of consecutive points
    assert res([(0, 0), (4, 0), (4, 3), (0, 3)]) == 1.5
    # the closing pair counts: (0, 1) -> (0, 0) is the shortest
    assert res([(0, 0), (10, 0), (10, 10), (0, 1)]) == 0.5
    # repeated points are skipped
    assert res([(0, 0), (0, 0), (6, 0), (6, 8)]) == 3.0
    # at least a 2048th of the longest side
    assert res([(0, 0), (0.001, 0), (4096, 0), (4096, 100)]) == 2.0
    assert res(np.array([[0.0, 0.0], [3.0, 4.0]])) == 2.5
    with pytest.raises(ValueError):
        res([(1, 1), (1, 1)])
    import math
    for key, ring, given in G.ring_cases():       # the vectorised rule against the point-by-point loop
        if given is None:
            d = [math.hypot(p[0] - q[0], p[1] - q[1]) for p, q in zip(np.roll(ring, 1, axis=0), ring)]
            assert res(ring) == max(0.5 * min(v for v in d if v > 0), np.max(np.ptp(ring, axis=0)) / 2048), key
