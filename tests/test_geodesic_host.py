"""CPU: the geodesic fixture (tests/golden/geodesic_v1.npz) against the restatements of
make_distance_map / shortest_path_in_distance_map / get_farthest_points that generated it, and the
plumbing of the GPU entry points (declared, bound, exported, loud without a GPU)."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("va_geodesic_workspace_bytes", "va_distance_map_i32", "va_distance_map_path",
                "va_farthest_points")


def _generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_geodesic", os.path.join(ROOT, "tests", "golden", "make_golden_geodesic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def geo():
    return np.load(os.path.join(ROOT, "tests", "golden", "geodesic_v1.npz"), allow_pickle=False)


def _ends(geo, name):
    e = geo[name + "/ends"]
    return [tuple(p) for p in e] if len(e) else None


def test_restatements_reproduce_the_fixture(geo):
    G = _generator()
    assert len(geo["names"]) >= 10
    for name in geo["names"]:
        mask = geo[name + "/mask"]
        starts = [tuple(p) for p in geo[name + "/starts"]]
        assert np.array_equal(G.distance_map(mask, starts, _ends(geo, name)), geo[name + "/map"]), name
        end = tuple(geo[name + "/path_end"])
        if end != (-1, -1):
            assert np.array_equal(G.shortest_path(geo[name + "/map"], end), geo[name + "/path"]), name
        fg = (mask != 0).astype(np.uint8)
        if fg.any():
            p1 = tuple(int(v) for v in geo[name + "/fp_p1_in"])
            a, b = G.farthest_points(fg, p1)
            assert np.array_equal(np.array([a, b]), geo[name + "/fp"]), name
            assert np.array_equal(G.farthest_points(fg, p1, ret_path=True), geo[name + "/fp_path"]), name


def test_restatement_follows_the_exact_pair_formula():
    """a check of the fixture generator's own restatement (not of the library): on an open square
    every value is 2 + a + floor(b * sqrt2) with b = min(x, y) diagonal and a = |x - y| straight steps"""
    G = _generator()
    m = np.ones((40, 40), np.int64)
    out = G.distance_map(m, [(0, 0)])
    yy, xx = np.mgrid[:40, :40]
    b = np.minimum(xx, yy)
    a = np.maximum(xx, yy) - b
    assert np.array_equal(out, 2 + a + np.floor(b * np.sqrt(2)).astype(np.int64))


def test_regions_exports_the_geodesic_functions():
    from video.analysis import regions
    for name in ("make_distance_map", "shortest_path_in_distance_map", "get_farthest_points"):
        assert callable(getattr(regions, name)), name


def test_geodesic_entry_points_are_declared_bound_and_exported():
    from video import _hip
    text = open(os.path.join(ROOT, "include", "videoanalysis_hip.h")).read()
    lib = _hip.load_library()
    for name in ENTRY_POINTS:
        assert name + "(" in text, name
        assert name in _hip.SIGNATURES, name
        assert hasattr(lib, name), name


def test_make_distance_map_rejects_other_dtypes():
    from video.analysis import regions
    with pytest.raises(TypeError):
        regions.make_distance_map(np.ones((4, 4), np.uint8), [(0, 0)])
    with pytest.raises(TypeError):
        regions.make_distance_map(np.ones((4, 4), np.float64), [(0, 0)])


def test_geodesic_ops_fail_loudly_without_gpu():
    from video import _hip
    if _hip.gpu_available():
        pytest.skip("a GPU is present")
    from video import ops
    from video.analysis import regions
    m = np.ones((8, 8), np.int64)
    with pytest.raises(_hip.HipUnavailableError):
        regions.make_distance_map(m, [(0, 0)])
    with pytest.raises(_hip.HipUnavailableError):
        regions.shortest_path_in_distance_map(m + 1, (3, 3))
    with pytest.raises(_hip.HipUnavailableError):
        regions.get_farthest_points(np.ones((8, 8), np.uint8))
    with pytest.raises(_hip.HipUnavailableError):
        ops.farthest_points(np.ones((2, 8, 8), np.uint8))
