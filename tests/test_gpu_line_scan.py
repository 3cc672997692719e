"""GPU: batched 8-bit affine warps (va_line_scan_u8, va_warp_affine_u8) and line_scan / line_scans / get_subimage of
video.analysis.image against the NumPy restatement of tests/golden/make_golden_line_scan.py and the reference-run
fixture line_scan_v1.npz.  Everything is compared with np.array_equal.  Reads the npz and the generator's
restatement only."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_line_scan", os.path.join(ROOT, "tests", "golden", "make_golden_line_scan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()


@pytest.fixture(scope="module")
def fx():
    from video import _hip
    _hip.lib()
    return np.load(os.path.join(ROOT, "tests", "golden", "line_scan_v1.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def batch():
    """(frames, frame index, p1, p2, half widths, restated strips) of the ragged batch"""
    frames, cases = G.gpu_frames(), G.gpu_batch()
    strips = [G.line_scan_strip(frames[f], p1, p2, hw)[1] for f, p1, p2, hw in cases]
    return (frames, np.array([c[0] for c in cases]), np.array([c[1] for c in cases], np.float64),
            np.array([c[2] for c in cases], np.float64), np.array([c[3] for c in cases], np.float64), strips)


def _rotation(angle_deg, src_shape, dst_shape):
    """forward matrix of a rotation about the source's centre that lands on the destination's centre"""
    a = math.radians(angle_deg)
    c, s = math.cos(a), math.sin(a)
    cx, cy = (src_shape[1] - 1) / 2.0, (src_shape[0] - 1) / 2.0
    dx, dy = (dst_shape[1] - 1) / 2.0, (dst_shape[0] - 1) / 2.0
    return np.array([[c, s, dx - c * cx - s * cy], [-s, c, dy + s * cx - c * cy]])


# ------------------------------------------------------------------------------------------ line scans
def test_ragged_batch_equals_restatement(batch):
    from video import ops
    frames, fidx, p1, p2, hw, strips = batch
    assert frames.shape == (3, 47, 61) and len(strips) >= 400
    assert set(G.GPU_LENGTHS) <= {s.shape[1] for s in strips}
    assert {int(2 * w) for w in G.GPU_HALF_WIDTHS} <= {s.shape[0] for s in strips}
    assert any(not s.any() for s in strips)                                  # a scan wholly outside
    assert any(s.min() == 255 for s, f in zip(strips, fidx) if f == 2)       # the top of the range survives rounding
    assert any(0 < np.count_nonzero(s) < s.size for s, f in zip(strips, fidx) if f == 2)    # and meets the border
    assert p1.min() < 0 and p2.min() < 0                                     # negative coordinates
    keep = frames.copy(), fidx.copy(), p1.copy(), p2.copy(), hw.copy()
    profiles, sums = ops.line_scans(frames, p1, p2, hw, frame_index=fidx, ret_sums=True)
    assert len(profiles) == len(sums) == len(strips)
    for k, (prof, sm, strip) in enumerate(zip(profiles, sums, strips)):
        assert sm.dtype == np.int32 and sm.shape == (strip.shape[1],), k
        assert np.array_equal(sm, strip.sum(axis=0, dtype=np.int64)), k
        assert prof.dtype == np.float64 and np.array_equal(prof, strip.mean(axis=0)), k
    for got, want in zip((frames, fidx, p1, p2, hw), keep):                  # the inputs are left alone
        assert np.array_equal(got, want)
    again = ops.line_scans(frames, p1, p2, hw, frame_index=fidx)             # without the sums: the same profiles
    assert all(np.array_equal(a, b) for a, b in zip(again, profiles))


def test_each_scan_alone_equals_batched(batch):
    from video import ops
    frames, fidx, p1, p2, hw, strips = batch
    for k, strip in enumerate(strips):
        got = ops.line_scans(frames[fidx[k]], p1[k:k + 1], p2[k:k + 1], float(hw[k]))
        assert len(got) == 1 and np.array_equal(got[0], strip.mean(axis=0)), k


def test_long_scan_has_many_chunks():
    """more than one workgroup's worth of chunks for one scan, on a frame whose rows are no multiple of 4 bytes"""
    from video import ops
    frame = np.random.default_rng(41).integers(0, 256, (203, 1003), dtype=np.uint8)
    cases = [((1.5, 100.25), (1001.0, 120.0), 5), ((990, 3), (4, 199), 2.5), ((500, 0), (500, 202), 7)]
    got = ops.line_scans(frame, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
    for k, (a, b, w) in enumerate(cases):
        assert np.array_equal(got[k], G.line_scan(frame, a, b, w)), k
    assert len(got[0]) == 999 and len(got[1]) > 5 * 64 * 3


# ----------------------------------------------------------------------------------------------- warps
def test_warp_affine_ragged_sizes_with_and_without_the_inverse_flag():
    from video import ops
    rng = np.random.default_rng(42)
    frames = rng.integers(0, 256, (2, 240, 323), dtype=np.uint8)
    sizes = [(1, 1), (1, 70), (70, 1), (33, 65), (300, 500), (16, 64), (17, 128)]
    mats = [_rotation(10.0 * k + 7, frames.shape[1:], s) for k, s in enumerate(sizes)]
    mats[4] = _rotation(30.0, frames.shape[1:], sizes[4])
    mats[5] = np.array([[1.0, 0.0, -100.0], [0.0, 1.0, -50.0]])               # an exact crop
    fidx = [0, 1, 0, 1, 1, 0, 1]
    want = [G.warp_affine(frames[f], M, (s[1], s[0])) for f, M, s in zip(fidx, mats, sizes)]
    assert np.array_equal(want[5], frames[0, 50:66, 100:164])
    assert want[4].any() and not want[4][0, 0] and not want[4][-1, -1]        # the rotated frame's corners are border
    keep = frames.copy()
    got = ops.warp_affine(frames, mats, sizes, frame_index=fidx)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.uint8 and g.shape == sizes[k] and np.array_equal(g, w), k
    inv = [G.invert(M) for M in mats]
    got = ops.warp_affine(frames, inv, sizes, frame_index=fidx, inverse=True)
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), k
    # mixed flags in one call, and a single frame without an index
    flags = [k % 2 == 1 for k in range(len(sizes))]
    got = ops.warp_affine(frames, [i if f else M for M, i, f in zip(mats, inv, flags)], sizes, frame_index=fidx,
                          inverse=flags)
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), k
    one = ops.warp_affine(frames[1], mats[4], [sizes[4]])
    assert len(one) == 1 and np.array_equal(one[0], want[4])
    assert np.array_equal(frames, keep)


# ------------------------------------------------------------------------------------- the public layer
def test_image_functions_equal_fixture(fx):
    from video.analysis import image
    imgs = {n: fx["image/%s" % n] for n in G.images()}
    by_image = {}
    for k, (name, p1, p2, hw) in enumerate(G.SCAN_CASES):
        got = image.line_scan(imgs[name], p1, p2, hw)
        assert got.dtype == np.float64 and np.array_equal(got, fx["scan/%d/profile" % k]), k
        by_image.setdefault((name, hw), []).append(k)
    for (name, hw), ks in by_image.items():
        got = image.line_scans(imgs[name], [G.SCAN_CASES[k][1] for k in ks], [G.SCAN_CASES[k][2] for k in ks], hw)
        for k, g in zip(ks, got):
            assert np.array_equal(g, fx["scan/%d/profile" % k]), k
    # a stack: per-frame point lists in, per-frame profile lists out
    stack = np.stack([imgs["noise"], imgs["ramp"], imgs["noise"]])
    ks = [[k for k, c in enumerate(G.SCAN_CASES) if c[0] == n and c[3] == 5] for n in ("noise", "ramp")] + [[]]
    got = image.line_scans(stack, [[G.SCAN_CASES[k][1] for k in f] for f in ks],
                           [[G.SCAN_CASES[k][2] for k in f] for f in ks], 5)
    assert [len(g) for g in got] == [len(f) for f in ks] and len(ks[0]) >= 2 and len(ks[1]) >= 2
    for f, g in zip(ks, got):
        for k, prof in zip(f, g):
            assert np.array_equal(prof, fx["scan/%d/profile" % k]), k
    for k, (name, sx, sy, width, height) in enumerate(G.SUBIMAGE_CASES):
        got = image.get_subimage(imgs[name], sx, sy, width, height)
        want = fx["sub/%d/image" % k]
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), k
    sub = image.get_subimage(imgs["noise"], (10, 50), (5, 35))
    assert np.array_equal(sub.T, imgs["noise"][5:35, 10:50])                 # the reference's transposed crop


# -------------------------------------------------------------------------------- limits and streams
def test_error_codes_and_per_item_status():
    from video import _hip, ops
    from video._hip import DeviceBuffer
    L = _hip.lib()
    N = None
    assert L.va_line_scan_u8(N, 1, 0, 8, 0, N, N, N, N, N, 0, 0, N, N, N) == -22             # h == 0
    assert L.va_line_scan_u8(N, -1, 8, 8, 0, N, N, N, N, N, 0, 0, N, N, N) == -22
    assert L.va_line_scan_u8(N, 1, 8, 8, -1, N, N, N, N, N, 0, 0, N, N, N) == -22
    assert L.va_line_scan_u8(N, 1, 8, 8, 0, N, N, N, N, N, 0, -1, N, N, N) == -22
    assert L.va_line_scan_u8(N, 1, 8, 8, 2, N, N, N, N, N, 1, 0, N, N, N) == -22             # fewer work items than items
    assert L.va_line_scan_u8(N, 1, 1 << 15, 1 << 14, 0, N, N, N, N, N, 0, 0, N, N, N) == -22   # 2^29 pixels
    assert L.va_line_scan_u8(N, 1, 8, 8, 1, N, N, N, N, N, 1, 0, N, N, N) == -22             # NULL
    assert b"NULL" in L.va_last_error()
    assert L.va_line_scan_u8(N, 1, 8, 8, 0, N, N, N, N, N, 0, 0, N, N, N) == 0
    assert L.va_warp_affine_u8(N, 1, 8, 0, 0, N, N, N, N, N, N, 0, 0, N, N, N) == -22
    assert L.va_warp_affine_u8(N, 1, 8, 8, -1, N, N, N, N, N, N, 0, 0, N, N, N) == -22
    assert L.va_warp_affine_u8(N, 1, 8, 8, 2, N, N, N, N, N, N, 1, 0, N, N, N) == -22
    assert L.va_warp_affine_u8(N, 1, 8, 8, 1, N, N, N, N, N, N, 1, 0, N, N, N) == -22
    assert L.va_warp_affine_u8(N, 1, 8, 8, 0, N, N, N, N, N, N, 0, 0, N, N, N) == 0

    frames = G.gpu_frames()
    n, h, w = frames.shape
    good = [(0, (10, 30), (50, 30), 3), (1, (10, 30), (10, 5), 2), (2, (20, 20), (30.5, 20), 1)]
    geo = [G.scan_geometry(p1, p2, hw) for _, p1, p2, hw in good]
    gm = [G.get_affine_transform(s, d) for s, d, _, _ in geo]
    tiny = np.array([[1e-9, 0.0, 0.0], [0.0, 1e-9, 0.0]])                    # its inverse leaves int32
    nan = np.array([[1.0, 0.0, np.nan], [0.0, 1.0, 0.0]])
    #         frame  matrix  rows   cols  offset
    items = [(0, gm[0], 6, 40, 0),               # runs
             (0, gm[0], 40000, 10, 40),          # a side above 32767
             (1, gm[1], 4, 25, 50),              # runs
             (0, tiny, 2, 10, 75),               # a coordinate beyond the limit
             (0, gm[0], 6, 10, 10 ** 6),         # an offset beyond the buffer
             (3, gm[0], 6, 10, 85),              # a frame index beyond the stack
             (0, gm[0], 6, -1, 85),              # a negative side
             (2, gm[2], 2, 10, 95),              # runs
             (0, nan, 2, 5, 105),                # not a number
             (0, gm[0], 6, 40, 108)]             # the range ends beyond the buffer
    total = 110
    m = len(items)
    fb, ib, mb, sb, ob, pb = (DeviceBuffer.from_array(a) for a in (
        frames, np.array([i[0] for i in items], np.int32), np.stack([i[1] for i in items]),
        np.array([[i[2], i[3]] for i in items], np.int32), np.array([i[4] for i in items], np.int64),
        np.arange(m, dtype=np.int32)))
    out, st = DeviceBuffer.from_array(np.full(total, 77, np.int32)), DeviceBuffer.from_array(np.full(m, 5, np.int32))
    assert L.va_line_scan_u8(fb.ptr, n, h, w, m, ib.ptr, mb.ptr, sb.ptr, ob.ptr, pb.ptr, m, total, out.ptr, st.ptr,
                             None) == 0
    assert st.download((m,), np.int32).tolist() == [0, -34, 0, -34, -34, -34, -34, 0, -34, -34]
    want = np.full(total, 77, np.int32)
    for k, o in ((0, 0), (1, 50), (2, 95)):
        f, p1, p2, hw = good[k]
        strip = G.line_scan_strip(frames[f], p1, p2, hw)[1]
        want[o:o + strip.shape[1]] = strip.sum(axis=0)
    assert np.array_equal(out.download((total,), np.int32), want)            # refused ranges keep their 77s

    # the same for warps: (frame, matrix, dh, dw, flag, offset)
    crop = np.array([[1.0, 0.0, -5.0], [0.0, 1.0, -7.0]])
    witems = [(0, crop, 5, 7, 0, 0), (0, crop, 40000, 1, 0, 35), (1, G.invert(crop), 20, 70, 1, 35),
              (0, tiny, 3, 3, 0, 1435), (0, tiny, 3, 3, 1, 1435), (2, crop, 3, 4, 0, 1444), (1, crop, 3, 4, 0, 1450)]
    total = 1456
    m = len(witems)
    tiles = np.array([1, 1, 4, 1, 1, 1, 1], np.int64)
    prefix = np.concatenate([[0], np.cumsum(tiles)[:-1]]).astype(np.int32)
    ib, mb, sb, gb, ob, pb = (DeviceBuffer.from_array(a) for a in (
        np.array([i[0] for i in witems], np.int32), np.stack([i[1] for i in witems]),
        np.array([[i[2], i[3]] for i in witems], np.int32), np.array([i[4] for i in witems], np.int32),
        np.array([i[5] for i in witems], np.int64), prefix))
    out, st = DeviceBuffer.from_array(np.full(total, 77, np.uint8)), DeviceBuffer.from_array(np.full(m, 5, np.int32))
    assert L.va_warp_affine_u8(fb.ptr, n, h, w, m, ib.ptr, mb.ptr, sb.ptr, gb.ptr, ob.ptr, pb.ptr, int(tiles.sum()),
                               total, out.ptr, st.ptr, None) == 0
    # tiny as an inverse map is within the limits: every pixel reads the source's corner
    assert st.download((m,), np.int32).tolist() == [0, -34, 0, -34, 0, 0, -34]
    got = out.download((total,), np.uint8)
    assert np.array_equal(got[:35].reshape(5, 7), frames[0, 7:12, 5:12])
    assert np.array_equal(got[35:1435].reshape(20, 70), G.warp_affine(frames[1], crop, (70, 20)))
    assert np.array_equal(got[1435:1444], np.full(9, frames[0, 0, 0]))
    assert np.array_equal(got[1444:1456].reshape(3, 4), frames[2, 7:10, 5:9])       # the last item left it alone

    # through ops: a refused item raises
    with pytest.raises(ValueError, match="limits"):
        ops.line_scans(frames[0], [(2e6, 2e6)], [(2e6 + 10, 2e6)])
    with pytest.raises(ValueError, match="limits"):
        ops.warp_affine(frames[0], [crop, tiny], [(3, 3), (3, 3)])


def test_created_stream_back_to_back(batch):
    from video import _hip, ops
    frames, fidx, p1, p2, hw, strips = batch
    L = _hip.lib()
    s = C.c_void_p()
    assert L.va_stream_create(C.byref(s)) == 0
    try:
        a, b = slice(0, 150), slice(150, 400)
        M = _rotation(30.0, frames.shape[1:], (40, 90))
        got_a = ops.line_scans(frames, p1[a], p2[a], hw[a], frame_index=fidx[a], stream=s.value)
        got_w = ops.warp_affine(frames, [M, M], [(40, 90), (40, 90)], frame_index=[0, 2], stream=s.value)
        got_b = ops.line_scans(frames, p1[b], p2[b], hw[b], frame_index=fidx[b], stream=s.value)
        for g, strip in zip(got_a + got_b, strips[:400]):
            assert np.array_equal(g, strip.mean(axis=0))
        assert np.array_equal(got_w[0], G.warp_affine(frames[0], M, (90, 40)))
        assert np.array_equal(got_w[1], G.warp_affine(frames[2], M, (90, 40)))
    finally:
        L.va_stream_destroy(s.value)
