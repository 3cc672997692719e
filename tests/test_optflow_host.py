"""CPU: the optical-flow fixture (tests/golden/optflow_v1.npz) is complete and its NumPy restatement reproduces
it bit for bit; the library's host-side Farneback constants equal the restatement's; the restatement is a
working optical flow; FilterOpticalFlow exists and fails loudly without a GPU."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gen():
    spec = importlib.util.spec_from_file_location(
        "make_golden_optflow", os.path.join(ROOT, "tests", "golden", "make_golden_optflow.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _gen()


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "optflow_v1.npz"), allow_pickle=False)


def test_fixture_is_complete(fixture):
    keys = set(fixture.files)
    for n, s in G.POLY_CONSTS:
        for part in ("g", "xg", "xxg", "ig"):
            assert "consts_%d_%g_%s" % (n, s, part) in keys
    for name, n, h, w, seed, step, dtype, extra, full in G.CASES:
        parts = ("frames", "flow", "mag") if full else ("frames_sha", "flow_sha", "mag_sha", "mag_sample",
                                                        "flow_sample")
        for part in parts:
            assert name + "_" + part in keys, name + "_" + part
        if full:
            assert fixture[name + "_flow"].shape == (n - 1, h, w, 2)
            assert fixture[name + "_mag"].dtype == np.float32
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "optflow_v1.npz")) < 512 * 1024


def test_restatement_reproduces_fixture(fixture):
    fresh = G.make()
    assert sorted(fresh) == sorted(fixture.files)
    for k in fixture.files:
        assert fresh[k].dtype == fixture[k].dtype, k
        assert np.array_equal(fresh[k], fixture[k]), k


def test_level_plan_of_the_reference_parameters():
    plan = G.level_plan(1080, 1920, 0.5, 3)
    assert [p[3] for p in plan] == [19, 9, 3, 3]                      # ksize of levels 3, 2, 1, 0
    assert [(p[4], p[5]) for p in plan] == [(135, 240), (270, 480), (540, 960), (1080, 1920)]
    assert len(G.level_plan(40, 50, 0.5, 3)) == 1                     # the 32-pixel rule: levels = 0


def test_poly_consts_of_the_library_match_restatement(fixture):
    from video import _hip
    for n, s in G.POLY_CONSTS:
        g, xg, xxg, ig = _hip.farneback_poly_consts(n, s)
        key = "consts_%d_%g_" % (n, s)
        assert np.array_equal(g, fixture[key + "g"])
        assert np.array_equal(xg, fixture[key + "xg"])
        assert np.array_equal(xxg, fixture[key + "xxg"])
        assert np.array_equal(np.array(ig), fixture[key + "ig"])
    with pytest.raises(_hip.HipError, match="poly_n must be 5 or 7"):
        _hip.farneback_poly_consts(6, 1.2)


@pytest.mark.parametrize("shift", [(1.0, 0.0), (0.0, 2.0), (1.5, -0.5)])
def test_restatement_measures_a_known_shift(shift):
    a = G.smooth_texture(96, 128, (0.0, 0.0))
    b = G.smooth_texture(96, 128, shift)
    flow = G.farneback(a, b, **G.REFERENCE_PARAMS)
    inner = (slice(10, -10), slice(10, -10))
    mag = G.magnitude(flow)[inner]
    assert abs(np.median(mag) - np.hypot(*shift)) < 0.1
    assert abs(np.median(flow[inner][..., 0]) - shift[0]) < 0.1
    assert abs(np.median(flow[inner][..., 1]) - shift[1]) < 0.1


def test_filter_imports_and_needs_a_gpu():
    from video import _hip
    from video.filters import FilterOpticalFlow
    from video.io.memory import VideoMemory
    v = FilterOpticalFlow(VideoMemory(np.zeros((5, 40, 48), np.uint8)))
    assert v.frame_count == 4
    if _hip.gpu_available():
        pytest.skip("a GPU is present")
    with pytest.raises(_hip.HipUnavailableError):
        next(iter(v))
    from video import ops
    with pytest.raises(_hip.HipUnavailableError):
        ops.optical_flow_farneback(np.zeros((2, 40, 48), np.uint8))
