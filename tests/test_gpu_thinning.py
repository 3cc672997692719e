"""GPU: Guo-Hall thinning (va_guo_hall_thinning_batch, va_guo_hall_thinning_u8) and the `guo-hall` method of
mask_thinning / Polygon.get_skeleton against the NumPy restatement of tests/golden/make_golden_thinning.py and the
reference-run fixture thinning_v1.npz.  Everything is compared with np.array_equal, iteration counts included.
Reads the npz and the generator's restatement only."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_thinning", os.path.join(ROOT, "tests", "golden", "make_golden_thinning.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()


@pytest.fixture(scope="module")
def fx():
    from video import _hip
    _hip.lib()
    return np.load(os.path.join(ROOT, "tests", "golden", "thinning_v1.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def batch():
    """(names, masks, restated skeletons, restated iteration counts) of the ragged batch"""
    cases = G.resident_batch()
    want = [G.guo_hall(m) for _, m in cases]
    return [n for n, _ in cases], [m for _, m in cases], [s for s, _ in want], np.array([i for _, i in want], np.int32)


def _same(got, want, names):
    for n, g, w in zip(names, got, want):
        assert g.dtype == np.uint8 and g.shape == w.shape and np.array_equal(g, w), n


# --------------------------------------------------------------------------------------------- resident
def test_ragged_batch_equals_restatement(batch):
    from video import ops
    names, masks, skels, iters = batch
    assert len(masks) >= 300
    assert max(ops._thin_words(m.shape) for m in masks) == ops.THIN_RESIDENT_MAX_WORDS
    assert {m.shape[1] for m in masks} >= set(range(1, 71))
    keep = [m.copy() for m in masks]
    got, it = ops.guo_hall_thinning(masks, implementation="resident", ret_iterations=True)
    _same(got, skels, names)
    assert it.dtype == np.int32 and it.tolist() == iters.tolist()
    for n, m, k in zip(names, masks, keep):                             # the inputs are left alone
        assert m.dtype == k.dtype and np.array_equal(m, k), n
    _same(ops.guo_hall_thinning(masks), skels, names)                   # the default: the largest go tiled


def test_one_at_a_time_equals_batched(batch):
    from video import ops
    names, masks, skels, iters = batch
    for k in range(len(masks)):
        got, it = ops.guo_hall_thinning([masks[k]], implementation="resident", ret_iterations=True)
        assert np.array_equal(got[0], skels[k]) and int(it[0]) == int(iters[k]), names[k]


def test_fixture_masks(fx):
    from video import ops
    names = list(G.fixture_masks())
    for impl in ("resident", "tiled"):
        got, it = ops.guo_hall_thinning([fx["mask/%s" % n] for n in names], implementation=impl, ret_iterations=True)
        _same(got, [fx["skel/%s" % n] for n in names], names)
        assert it.tolist() == [int(fx["iters/%s" % n]) for n in names], impl


def test_empty_list_and_stacks():
    from video import ops
    assert ops.guo_hall_thinning([]) == []
    stack = np.stack([G.blob(40 + k, 50, 77, 3.0, -0.2 * k) for k in range(5)])
    want = [G.guo_hall(f) for f in stack]
    for impl in (None, "resident", "tiled"):
        got, it = ops.guo_hall_thinning(stack, implementation=impl, ret_iterations=True)
        assert isinstance(got, np.ndarray) and got.shape == stack.shape and got.dtype == np.uint8
        assert np.array_equal(got, np.stack([s for s, _ in want])) and it.tolist() == [i for _, i in want], impl
    got = ops.guo_hall_thinning(stack.astype(bool))
    assert got.dtype == np.uint8 and np.array_equal(got, np.stack([s for s, _ in want]))
    assert ops.guo_hall_thinning(np.zeros((0, 4, 4), np.uint8)).shape == (0, 4, 4)


# ------------------------------------------------------------------------------------------------ tiled
def test_tiled_equals_resident_and_restatement(batch):
    from video import ops
    names, masks, skels, iters = batch
    got, it = ops.guo_hall_thinning(masks, implementation="tiled", ret_iterations=True)
    _same(got, skels, names)
    assert it.tolist() == iters.tolist()
    res, it_res = ops.guo_hall_thinning(masks, implementation="resident", ret_iterations=True)
    _same(got, res, names)
    assert it.tolist() == it_res.tolist()


@pytest.mark.parametrize("k_sub,poll", [(0, 0), (2, 1), (4, 3), (6, 2), (16, 1), (8, 64)])
def test_tiled_launch_parameters_do_not_change_the_result(k_sub, poll):
    from video import ops
    # sizes that are no multiples of the tile (64 - 2 K rows, 448 columns) or of a word; iteration counts that are
    # no multiples of K / 2 or of the polling period's K / 2 * poll
    stack = np.stack([G.blob(810 + k, 203, 1003, 2.5 + 1.5 * k, -0.2) for k in range(3)])
    want = [G.guo_hall(f) for f in stack]
    counts = [i for _, i in want]
    assert len(set(counts)) == 3
    old = ops.THIN_TILED_SUB_ITERATIONS, ops.THIN_TILED_POLL
    ops.THIN_TILED_SUB_ITERATIONS, ops.THIN_TILED_POLL = k_sub, poll
    try:
        got, it = ops.guo_hall_thinning(stack, implementation="tiled", ret_iterations=True)
    finally:
        ops.THIN_TILED_SUB_ITERATIONS, ops.THIN_TILED_POLL = old
    assert np.array_equal(got, np.stack([s for s, _ in want])) and it.tolist() == counts
    per_launch = (k_sub or 16) // 2
    if per_launch > 1:
        assert any(c % per_launch for c in counts) and any(c % (per_launch * (poll or 2)) for c in counts)


def test_tiled_1080p_stack():
    from video import ops
    stack = np.stack([G.blob(900 + k, 1080, 1920, s, l) for k, (s, l) in
                      enumerate([(4.0, 0.0), (3.0, 0.3), (6.0, -0.5), (9.0, -0.8)])])
    stack[3] *= np.uint8(255)
    want = [G.guo_hall(f) for f in stack]
    counts = [i for _, i in want]
    assert len(set(counts)) >= 3                             # the frames converge at different iterations
    got, it = ops.guo_hall_thinning(stack, ret_iterations=True)          # too large for LDS: the tiled path
    assert it.tolist() == counts
    for k in range(4):
        assert np.array_equal(got[k], want[k][0]), k
    with pytest.raises(ValueError):
        ops.guo_hall_thinning(stack[:1], implementation="resident")
    one = ops.guo_hall_thinning([stack[1]])                  # one large mask of a list
    assert np.array_equal(one[0], want[1][0])


# ------------------------------------------------------------------------------------- the public layer
def test_mask_thinning_and_polygons_equal_fixture(fx):
    from video.analysis import shapes
    from video.analysis.image import mask_thinning
    for name in G.fixture_masks():
        mask = fx["mask/%s" % name]
        arg = mask.copy()
        got = mask_thinning(arg, "guo-hall")
        assert got.dtype == np.uint8 and np.array_equal(got, fx["skel/%s" % name]), name
        assert np.array_equal(arg, mask), name               # a new array: the argument is left alone
    polys = [shapes.Polygon(fx["poly/%s" % n]) for n in G.POLYGONS]
    for name, p in zip(G.POLYGONS, polys):
        assert np.array_equal(p.get_skeleton(method="guo-hall"), fx["skeleton/%s" % name]), name
        skel, off = p.get_skeleton(ret_offset=True, method="guo-hall")
        assert np.array_equal(skel, fx["skeleton5/%s" % name]), name
        assert tuple(off) == tuple(fx["skeleton5/%s/offset" % name]), name
        assert np.array_equal(p.get_skeleton_points(method="guo-hall"), fx["points/%s" % name]), name
    skels = shapes.get_skeletons(polys)
    with_off, offs = shapes.get_skeletons(polys, ret_offset=True)
    for name, p, s, s5, o in zip(G.POLYGONS, polys, skels, with_off, offs):
        assert np.array_equal(s, fx["skeleton/%s" % name]), name
        assert np.array_equal(s5, fx["skeleton5/%s" % name]) and tuple(o) == tuple(fx["skeleton5/%s/offset" % name])
        assert np.array_equal(s, p.get_skeleton(method="guo-hall"))
    assert shapes.get_skeletons([]) == []


def test_auto_and_python_are_unchanged(fx):
    from video import ops
    from video.analysis import shapes
    from video.analysis.image import mask_thinning
    for name in ("blob1", "worm0", "ring3", "comb4"):
        mask = fx["mask/%s" % name]
        want = ops.mask_thinning(mask)[0]
        assert np.array_equal(mask_thinning(mask), want), name
        assert np.array_equal(mask_thinning(mask, "auto"), want), name
        assert np.array_equal(mask_thinning(mask, "python"), want), name
        assert not np.array_equal(want, fx["skel/%s" % name]), name          # a different kind of skeleton
    p = shapes.Polygon(fx["poly/worm"])
    assert np.array_equal(p.get_skeleton(), ops.mask_thinning(p.get_mask())[0])
    assert np.array_equal(shapes.get_skeletons([p], method="python")[0], p.get_skeleton())


# -------------------------------------------------------------------------------- limits and streams
def test_error_codes_and_limits():
    from video import _hip
    from video._hip import DeviceBuffer
    L = _hip.lib()
    assert L.va_guo_hall_thinning_batch(None, None, None, 0, -1, 8, None, None, None, None) == -22
    assert L.va_guo_hall_thinning_batch(None, None, None, 0, 1, 15361, None, None, None, None) == -22
    assert L.va_guo_hall_thinning_batch(None, None, None, 0, 1, 8, None, None, None, None) == -22
    assert L.va_guo_hall_thinning_batch(None, None, None, 0, 0, 8, None, None, None, None) == 0
    assert L.va_guo_hall_thinning_u8(None, None, 0, None, 1, 8, 8, 0, 0, None, None, None) == -22
    assert L.va_guo_hall_thinning_u8(None, None, 0, None, 0, 8, 8, 3, 0, None, None, None) == -22
    assert L.va_guo_hall_thinning_u8(None, None, 0, None, 0, 8, 8, 18, 0, None, None, None) == -22
    assert L.va_guo_hall_thinning_u8(None, None, 0, None, 0, 8, 8, 0, 65, None, None, None) == -22
    assert L.va_guo_hall_thinning_u8(None, None, 0, None, 0, 0, 8, 0, 0, None, None, None) == -22
    assert L.va_guo_hall_thinning_u8(None, None, 0, None, 0, 8, 8, 0, 0, None, None, None) == 0
    assert L.va_guo_hall_thinning_u8(None, None, 0, None, 0, 65535 * 32 + 1, 8, 0, 0, None, None, None) == -22
    assert L.va_guo_hall_thinning_u8(None, None, 0, None, 4096, 1 << 20, 8, 0, 0, None, None, None) == -22
    assert L.va_guo_hall_thinning_scratch_bytes(1, 65535 * 32 + 1, 8) == 0
    assert L.va_guo_hall_thinning_scratch_bytes(0, 8, 8) == 0 and L.va_guo_hall_thinning_scratch_bytes(1, 8, 8) > 0
    src = DeviceBuffer.from_array(np.ones((8, 8), np.uint8))
    dst, small = DeviceBuffer(64), DeviceBuffer(16)
    assert L.va_guo_hall_thinning_u8(src.ptr, small.ptr, 16, dst.ptr, 1, 8, 8, 0, 0, None, None, None) == -22

    # per-item status: more words than max_words, an offset beyond the buffer, a negative side; the others run
    shapes = np.array([[5, 9], [3, 40], [5, 9], [-1, 4], [4, 6]], np.int32)
    offs = np.array([0, 45, 10 ** 6, 0, 165], np.int64)
    flat = np.ones(189, np.uint8)
    out0 = np.full(189, 77, np.uint8)
    mb, sb, ob, db = (DeviceBuffer.from_array(a) for a in (flat, shapes, offs, out0))
    ib, st = DeviceBuffer(20), DeviceBuffer(20)
    assert L.va_guo_hall_thinning_batch(mb.ptr, sb.ptr, ob.ptr, 189, 5, 5, db.ptr, ib.ptr, st.ptr, None) == 0
    assert st.download((5,), np.int32).tolist() == [0, -34, -34, -34, 0]
    out = db.download((189,), np.uint8)
    assert np.array_equal(out[:45].reshape(5, 9), G.guo_hall(np.ones((5, 9), np.uint8))[0])
    assert np.all(out[45:165] == 77)                                     # the refused item's box is not written
    assert np.array_equal(out[165:].reshape(4, 6), G.guo_hall(np.ones((4, 6), np.uint8))[0])
    its = ib.download((5,), np.int32)
    assert its[0] == 1 and its[4] == G.guo_hall(np.ones((4, 6), np.uint8))[1]


def test_created_stream_back_to_back():
    from video import _hip, ops
    L = _hip.lib()
    s = C.c_void_p()
    assert L.va_stream_create(C.byref(s)) == 0
    try:
        a = [G.blob(60 + k, 30 + 7 * k, 45 + 11 * k, 2.5, -0.2) for k in range(12)]
        b = np.stack([G.blob(80 + k, 140, 333, 3.0, -0.4) for k in range(3)])
        got_a = ops.guo_hall_thinning(a, stream=s.value)
        got_b = ops.guo_hall_thinning(b, implementation="tiled", stream=s.value)
        got_c = ops.guo_hall_thinning(a[::-1], stream=s.value)
        for m, g in zip(a, got_a):
            assert np.array_equal(g, G.guo_hall(m)[0])
        for m, g in zip(b, got_b):
            assert np.array_equal(g, G.guo_hall(m)[0])
        for m, g in zip(a[::-1], got_c):
            assert np.array_equal(g, G.guo_hall(m)[0])
    finally:
        L.va_stream_destroy(s.value)
