"""CPU: the Guo-Hall fixture (tests/golden/thinning_v1.npz), the NumPy restatement of the pinned definition
(tests/golden/make_golden_thinning.py) and the argument checks of the Python layer.  Needs no GPU and no
reference checkout.  The restatement is checked against the hand cases and against topological invariants
computed with SciPy's labelling."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPZ = os.path.join(ROOT, "tests", "golden", "thinning_v1.npz")


def _generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_thinning", os.path.join(ROOT, "tests", "golden", "make_golden_thinning.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()


@pytest.fixture(scope="module")
def fx():
    return np.load(NPZ, allow_pickle=False)


def test_fixture_is_complete(fx):
    assert len(fx["shims"]) >= 3
    for name in G.fixture_masks():
        for kind in ("mask", "skel", "iters"):
            assert "%s/%s" % (kind, name) in fx.files
    for name in G.POLYGONS:
        for kind in ("poly", "skeleton", "skeleton5", "points"):
            assert "%s/%s" % (kind, name) in fx.files
    assert os.path.getsize(NPZ) < 400 * 1024


def test_restatement_reproduces_fixture(fx):
    for name, mask in G.fixture_masks().items():
        assert np.array_equal(mask, fx["mask/%s" % name]), name
        keep = mask.copy()
        skel, it = G.guo_hall(mask)
        assert np.array_equal(mask, keep), name                      # the input is left alone
        assert skel.dtype == np.uint8 and np.array_equal(skel, fx["skel/%s" % name]), name
        assert it == int(fx["iters/%s" % name]), name


def test_polygon_skeletons_of_the_fixture_are_the_restatement_on_the_restated_masks(fx):
    for name in G.POLYGONS:
        c = fx["poly/%s" % name]
        assert np.array_equal(G.guo_hall(G.POL.get_mask(c, 0)[0])[0], fx["skeleton/%s" % name]), name
        mask, off = G.POL.get_mask(c, 5)
        skel = G.guo_hall(mask)[0]
        assert np.array_equal(skel, fx["skeleton5/%s" % name]) and off == tuple(fx["skeleton5/%s/offset" % name])
        y, x = np.nonzero(skel)
        assert np.array_equal(np.c_[x, y] + off, fx["points/%s" % name]), name


def test_hand_cases():
    # a 2x2 block at rows 1-2, columns 1-2 of a 4x4 field leaves the single pixel (1, 2) after 2 iterations
    m = np.zeros((4, 4), np.uint8)
    m[1:3, 1:3] = 1
    skel, it = G.guo_hall(m)
    assert it == 2 and np.argwhere(skel).tolist() == [[1, 2]]
    # a 3x7 bar at rows 1-3, columns 1-7 of a 5x9 field leaves row 2, columns 2-6, after 2 iterations
    m = np.zeros((5, 9), np.uint8)
    m[1:4, 1:8] = 1
    skel, it = G.guo_hall(m)
    want = np.zeros((5, 9), np.uint8)
    want[2, 2:7] = 1
    assert it == 2 and np.array_equal(skel, want)
    # an all-ones 5x9 field is unchanged after 1 iteration
    m = np.ones((5, 9), np.uint8)
    skel, it = G.guo_hall(m)
    assert it == 1 and np.array_equal(skel, m)
    # a plus of two 5-pixel arms in a 7x7 field is unchanged after 1 iteration
    m = np.zeros((7, 7), np.uint8)
    m[3, 1:6] = 1
    m[1:6, 3] = 1
    skel, it = G.guo_hall(m)
    assert it == 1 and np.array_equal(skel, m)
    for name, (mask, want, iters) in G.HAND_CASES.items():
        skel, it = G.guo_hall(mask)
        assert it == iters and np.array_equal(skel, want), name


def test_vector_form_equals_the_pixel_by_pixel_form():
    rng = np.random.default_rng(5)
    for k in range(30):
        h, w = int(rng.integers(1, 14)), int(rng.integers(1, 40))
        m = (rng.random((h, w)) < rng.uniform(0.3, 0.95)).astype(np.uint8) * np.uint8(rng.integers(1, 256))
        a, b = G.guo_hall(m), G.guo_hall_literal(m)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1], (h, w)


def test_invariants_on_seeded_blobs():
    from scipy import ndimage
    eight = np.ones((3, 3), int)
    rng = np.random.default_rng(11)
    for k in range(44):
        h, w = int(rng.integers(12, 120)), int(rng.integers(12, 150))
        m = G.blob(700 + k, h, w, float(rng.uniform(1.5, 5.0)), float(rng.uniform(-0.8, 0.4)))
        skel, it = G.guo_hall(m)
        assert not np.any(skel & ~m), k                                        # a subset of the mask
        assert ndimage.label(m, eight)[1] == ndimage.label(skel, eight)[1], k  # components kept
        assert ndimage.label(m == 0)[1] == ndimage.label(skel == 0)[1], k      # holes kept (4-connected complement)
        again, it2 = G.guo_hall(skel)
        assert it2 == 1 and np.array_equal(again, skel), k                     # a fixed point


def test_border_rule():
    m = np.pad(G.blob(31, 28, 40, 3.0, -0.3)[1:-1, 1:-1], 1, constant_values=1)
    skel, _ = G.guo_hall(m)
    assert skel[0].all() and skel[-1].all() and skel[:, 0].all() and skel[:, -1].all()
    assert skel.sum() < m.sum()
    rng = np.random.default_rng(2)
    for h, w in ((1, 1), (1, 7), (2, 7), (7, 1), (7, 2), (2, 2), (1, 40), (40, 2)):
        m = (rng.random((h, w)) < 0.8).astype(np.uint8) * np.uint8(7)
        skel, it = G.guo_hall(m)
        assert it == 1 and np.array_equal(skel, m), (h, w)


def test_argument_checks_need_no_gpu():
    from video import ops
    from video.analysis.image import mask_thinning
    ok = np.ones((5, 5), np.uint8)
    for bad in (np.float32, np.int32, np.uint16, np.int8):
        with pytest.raises(TypeError):
            ops.guo_hall_thinning([ok.astype(bad)])
        with pytest.raises(TypeError):
            mask_thinning(ok.astype(bad), "guo-hall")
    with pytest.raises(TypeError):
        ops.guo_hall_thinning(np.ones((2, 5, 5), np.float64))
    for bad in (np.ones(5, np.uint8), np.ones((1, 5, 5), np.uint8)):
        with pytest.raises(ValueError):
            ops.guo_hall_thinning([bad])
    with pytest.raises(ValueError):
        ops.guo_hall_thinning(ok)                                  # one 2-d array is neither a list nor a stack
    with pytest.raises(ValueError):
        ops.guo_hall_thinning(np.ones((2, 2, 5, 5), np.uint8))
    with pytest.raises(ValueError):
        ops.guo_hall_thinning([ok], implementation="lds")
    too_big = np.zeros((481, 1024), np.uint8)                      # 481 * 32 packed words
    assert ops._thin_words(too_big.shape) == ops.THIN_RESIDENT_MAX_WORDS + 32 == G.RESIDENT_MAX_WORDS + 32
    with pytest.raises(ValueError):
        ops.guo_hall_thinning([ok, too_big], implementation="resident")
    with pytest.raises(ValueError):
        ops.guo_hall_thinning(too_big[None], implementation="resident")
    with pytest.raises(ValueError):
        mask_thinning(ok, "zhang-suen")
    assert ops.guo_hall_thinning([]) == []
    skels, its = ops.guo_hall_thinning([], ret_iterations=True)
    assert skels == [] and its.dtype == np.int32 and its.shape == (0,)


def test_polygon_methods_pass_the_method_through():
    import inspect
    from video.analysis import shapes
    assert inspect.signature(shapes.Polygon.get_skeleton).parameters["method"].default == "auto"
    assert inspect.signature(shapes.Polygon.get_skeleton_points).parameters["method"].default == "auto"
    assert inspect.signature(shapes.get_skeletons).parameters["method"].default == "guo-hall"
    with pytest.raises(ValueError):
        shapes.get_skeletons([], method="zhang-suen")


def test_thinning_module_equals_restatement(fx):
    thinning = pytest.importorskip("thinning")
    for name in G.fixture_masks():
        arg = fx["mask/%s" % name].copy()
        assert np.array_equal(thinning.guo_hall_thinning(arg), fx["skel/%s" % name]), name
