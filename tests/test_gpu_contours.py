"""GPU: every outer contour of a frame stack (va_find_contours, ops.find_contours, regions.find_contours,
regions.get_external_contour) against the CPU oracle's Suzuki-Abe scanner, list for list and point for point, and
against the reference-run fixture contours_v1.npz.  Reads the npz and the generator's mask builders only."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_contours", os.path.join(ROOT, "tests", "golden", "make_golden_contours.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()
GUARD = 0xA5


@pytest.fixture(scope="module")
def fx():
    from video import _hip
    _hip.lib()
    return np.load(os.path.join(ROOT, "tests", "golden", "contours_v1.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def ops():
    from video import _hip, ops
    _hip.lib()
    return ops


@pytest.fixture(scope="module")
def batch(oracle):
    """the 9-frame batch and the oracle's lists for it, computed once"""
    stack = G.batch9()
    return stack, [oracle.find_contours_external_simple(m) for m in stack]


def same_lists(got, ref):
    return len(got) == len(ref) and all(a.shape == b.shape and a.dtype == np.int32 and np.array_equal(a, b)
                                        for a, b in zip(got, ref))


def raw(stack, cap_contours, cap_points, stream=None, slack=64):
    """va_find_contours through the C ABI into buffers `slack` entries larger than the capacities, filled with a
    guard byte; returns the raw arrays (whole buffers, guards included) and the return code"""
    from video import _hip
    from video.ops import CONTOUR_INFO_DTYPE
    from video._hip import DeviceBuffer
    L = _hip.lib()
    stack = np.ascontiguousarray(stack, np.uint8)
    n, h, w = stack.shape
    shapes = {"ncontours": ((n + slack,), np.int32), "totals": ((2 + slack,), np.int64),
              "info": ((cap_contours + slack,), CONTOUR_INFO_DTYPE), "point_off": ((cap_contours + 1 + slack,), np.int64),
              "points": ((cap_points + slack, 2), np.int32)}
    bufs = {k: DeviceBuffer.from_array(np.full(int(np.prod(s)) * np.dtype(t).itemsize, GUARD, np.uint8))
            for k, (s, t) in shapes.items()}
    src = DeviceBuffer.from_array(stack)
    ws_bytes = L.va_find_contours_workspace_bytes(n, h, w)
    ws = DeviceBuffer(ws_bytes)
    rc = L.va_find_contours(src.ptr, n, h, w, bufs["ncontours"].ptr, bufs["totals"].ptr, bufs["info"].ptr,
                            bufs["point_off"].ptr, cap_contours, bufs["points"].ptr, cap_points, ws.ptr, ws_bytes,
                            stream)
    _hip.check(L.va_stream_sync(stream))
    out = {k: bufs[k].download(*shapes[k]) for k in shapes}
    for b in list(bufs.values()) + [src, ws]:
        b.free()
    return rc, out


def guard_intact(a, used):
    """every byte of `a` beyond its first `used` entries still holds the guard pattern"""
    return bool(np.all(np.ascontiguousarray(a[used:]).view(np.uint8) == GUARD))


def lists_of(out, n):
    """per-frame lists from the raw buffers of a call with room for everything"""
    k, npts = (int(v) for v in out["totals"][:2])
    counts, off, pts = out["ncontours"][:n], out["point_off"][:k + 1], out["points"][:npts]
    first = np.concatenate([[0], np.cumsum(counts)])
    return [[pts[off[s]:off[s + 1]].reshape(-1, 1, 2) for s in range(first[f], first[f + 1])] for f in range(n)]


# ------------------------------------------------------------------------------- word boundaries
@pytest.mark.parametrize("w", G.WIDTHS)
def test_word_boundaries_of_the_start_detection(ops, oracle, w):
    for h in G.HEIGHTS:
        masks = np.stack([G.random_mask(1000 * w + 10 * h + int(10 * d), h, w, d) for d in G.DENSITIES])
        got = ops.find_contours(masks)
        for m, g in zip(masks, got):
            assert same_lists(g, oracle.find_contours_external_simple(m)), (h, w)
        assert ops.find_contours(np.zeros((h, w), np.uint8)) == []
        full = ops.find_contours(np.full((h, w), 255, np.uint8))
        assert same_lists(full, oracle.find_contours_external_simple(np.ones((h, w), np.uint8)))
        assert len(full) == 1 and len(full[0]) == (1 if h == w == 1 else 2 if 1 in (h, w) else 4)


def test_fixed_results(ops, fx):
    for name, (mask, sizes) in G.fixed_cases().items():
        got = ops.find_contours(mask)
        assert [len(c) for c in got] == sizes, name
        assert same_lists(got, G.unflatten(fx["c/fixed/%s/points" % name], fx["c/fixed/%s/sizes" % name])), name


# ---------------------------------------------------------------------------------- externality
def test_externality(ops, oracle):
    from scipy import ndimage
    fewer = 0
    for name, mask in G.externality_cases().items():
        got = ops.find_contours(mask)
        assert same_lists(got, oracle.find_contours_external_simple(mask)), name
        ncomp = ndimage.label(mask, structure=np.ones((3, 3), int))[1]
        assert len(got) <= ncomp, name
        fewer += len(got) < ncomp
        if name in ("diagonal_opening", "edge_ring"):
            assert len(got) == 1 and ncomp == 2, name      # the blob in the hole is not external
        if name == "column0":
            assert len(got) == 2 and got[0][0, 0].tolist() == [0, 3]      # the later start is listed first
        if name == "checkerboard":
            assert len(got) == 1 and ncomp == 1
    assert fewer >= 5      # the externality step is exercised: it removed contours


# ----------------------------------------------------------------------- order and ragged layout
def test_batch_order_and_ragged_layout(ops, batch):
    stack, ref = batch
    n = len(stack)
    assert [len(r) for r in ref][1] == 437 and len(ref[4]) == 0 and len(ref[8]) == 0
    total = sum(len(r) for r in ref)
    npts = sum(len(c) for r in ref for c in r)
    rc, out = raw(stack, total, npts)
    assert rc == 0
    assert out["totals"][:2].tolist() == [total, npts]
    assert out["ncontours"][:n].tolist() == [len(r) for r in ref]
    sizes = [len(c) for r in ref for c in r]
    assert np.array_equal(out["point_off"][:total + 1], np.concatenate([[0], np.cumsum(sizes)]))
    assert np.array_equal(out["info"]["npoints"][:total], sizes)
    frame_first = np.concatenate([[0], np.cumsum(out["ncontours"][:n])])
    for f in range(n):
        assert np.all(out["info"]["frame"][frame_first[f]:frame_first[f + 1]] == f)
    got = lists_of(out, n)
    for f in range(n):
        assert same_lists(got[f], ref[f]), f
        assert same_lists(ops.find_contours(stack[f]), ref[f]), f      # each frame alone
    assert all(guard_intact(out[k], used) for k, used in
               (("ncontours", n), ("totals", 2), ("info", total), ("point_off", total + 1), ("points", npts)))
    assert all(same_lists(g, r) for g, r in zip(ops.find_contours(stack), ref))


# ------------------------------------------------------------------------- per-contour records
def test_records_and_moments(ops, oracle, batch):
    from video import _hip
    from video._hip import DeviceBuffer
    from video.analysis.curves import curve_length
    stack, ref = batch
    contours, info, moments = ops.find_contours(stack, ret_info=True, moments=True)
    checked = 0
    for f in range(len(stack)):
        assert same_lists(contours[f], ref[f])
        assert len(info[f]) == len(moments[f]) == len(ref[f])
        for c, rec, mom in zip(ref[f], info[f], moments[f]):
            p = c.reshape(-1, 2)
            assert rec["area"] == oracle.contour_area(c)
            assert rec["perimeter"] == curve_length(np.concatenate([p, p[:1]]))
            x, y = p.min(axis=0)
            assert rec["rect"].tolist() == [x, y, p[:, 0].max() - x + 1, p[:, 1].max() - y + 1]
            want = oracle.contour_moments(c)
            assert mom.tolist() == [want[k] for k in oracle.MOMENT_KEYS[:10]]
            checked += 1
    assert checked > 600
    # the ragged moments equal va_contour_moments on the padded table
    flat = [c.reshape(-1, 2) for r in ref for c in r]
    cap = max(len(c) for c in flat)
    table = np.zeros((len(flat), cap, 2), np.int32)
    for k, c in enumerate(flat):
        table[k, :len(c)] = c
    L = _hip.lib()
    tb, nb, mb = (DeviceBuffer.from_array(table), DeviceBuffer.from_array(np.array([len(c) for c in flat], np.int32)),
                  DeviceBuffer(len(flat) * 80))
    _hip.check(L.va_contour_moments(tb.ptr, nb.ptr, len(flat), cap, 0, mb.ptr, None))
    padded = mb.download((len(flat), 10), np.float64)
    assert np.array_equal(padded.view(np.uint64), np.concatenate([m for m in moments if len(m)]).view(np.uint64))
    # float32 points through the ragged entry point
    pts = np.concatenate(flat).astype(np.float32) + np.float32(0.25)
    off = np.concatenate([[0], np.cumsum([len(c) for c in flat])]).astype(np.int64)
    pb, ob = DeviceBuffer.from_array(pts), DeviceBuffer.from_array(off)
    _hip.check(L.va_contour_moments_ragged(pb.ptr, ob.ptr, len(flat), 1, mb.ptr, None))
    got = mb.download((len(flat), 10), np.float64)
    for k in (0, 1, len(flat) // 2, len(flat) - 1):
        want = oracle.contour_moments(pts[off[k]:off[k + 1]])
        assert got[k].tolist() == [want[key] for key in oracle.MOMENT_KEYS[:10]]
    for b in (tb, nb, mb, pb, ob):
        b.free()


# ---------------------------------------------------------------------------------- capacities
@pytest.mark.parametrize("cap_contours,cap_points", [(50, 300), (700, 300), (50, 100000), (0, 0), (100, 566)])
def test_capacities(batch, cap_contours, cap_points):
    stack, ref = batch
    n = len(stack)
    flat = [c for r in ref for c in r]
    total, npts = len(flat), sum(len(c) for c in flat)
    rc, out = raw(stack, cap_contours, cap_points)
    assert rc == 0                                                # exceeding a capacity is no error
    assert out["totals"][:2].tolist() == [total, npts]            # the true totals
    assert out["ncontours"][:n].tolist() == [len(r) for r in ref]
    slots = min(total, cap_contours)
    off = np.concatenate([[0], np.cumsum([len(c) for c in flat])])
    assert np.array_equal(out["point_off"][:slots + 1], off[:slots + 1])
    assert np.array_equal(out["info"]["npoints"][:slots], [len(c) for c in flat[:slots]])
    # the contours that fit whole form a prefix; each of them is complete, nothing follows them
    fit = sum(1 for s in range(slots) if off[s + 1] <= cap_points)
    for s in range(fit):
        assert np.array_equal(out["points"][off[s]:off[s + 1]], flat[s].reshape(-1, 2)), s
    assert guard_intact(out["points"], off[fit])
    assert all(guard_intact(out[k], used) for k, used in
               (("ncontours", n), ("totals", 2), ("info", slots), ("point_off", slots + 1)))


def test_tiny_default_capacities_rerun_exactly_once(ops, batch, monkeypatch):
    from video import _hip
    stack, ref = batch
    L = _hip.lib()
    calls = []

    class Counting(object):
        def __getattr__(self, name):
            fn = getattr(L, name)
            if name != "va_find_contours":
                return fn

            def counted(*a):
                calls.append(a[8:11:2])
                return fn(*a)
            return counted
    monkeypatch.setattr(ops._hip, "lib", lambda *a: Counting())
    for capc, capp in ((3, 1 << 17), (4096, 5), (3, 5)):
        monkeypatch.setattr(ops, "DEFAULT_CONTOUR_CAPACITY", capc)
        monkeypatch.setattr(ops, "DEFAULT_CONTOUR_POINT_CAPACITY", capp)
        del calls[:]
        got = ops.find_contours(stack)
        assert all(same_lists(g, r) for g, r in zip(got, ref))
        total, npts = sum(len(r) for r in ref), sum(len(c) for r in ref for c in r)
        assert calls == [(capc, capp), (total, npts)]
    monkeypatch.undo()
    del calls[:]
    assert all(same_lists(g, r) for g, r in zip(ops.find_contours(stack), ref))


# ------------------------------------------------------------------------------ labelling paths
@pytest.mark.parametrize("path,lds_runs", [(1, 0), (2, 0), (4, 0), (2, 7)])
def test_labelling_paths(ops, batch, path, lds_runs):
    from video import _hip
    stack, ref = batch
    _hip.check(_hip.lib().va_test_hook_labelling(path, lds_runs))
    try:
        got = ops.find_contours(stack)
    finally:
        _hip.check(_hip.lib().va_test_hook_labelling(0, 0))
    assert all(same_lists(g, r) for g, r in zip(got, ref))


# ---------------------------------------------------------------------------------- mid-size
def test_blob_masks(ops, fx, oracle):
    stack = G.blob_stack()
    got, info = ops.find_contours(stack, ret_info=True)
    longest = 0
    for f, m in enumerate(stack):
        ref = G.unflatten(fx["c/blobs/%d/points" % f], fx["c/blobs/%d/sizes" % f])
        assert same_lists(got[f], ref), f
        assert same_lists(got[f], oracle.find_contours_external_simple(m)), f
        assert [r["area"] for r in info[f]] == [oracle.contour_area(c) for c in ref]
        longest = max(longest, float(info[f]["perimeter"].max()))
    assert longest > 1500      # walks of a few thousand steps


# ------------------------------------------------------------------- scans over more than a wave
def test_scans_with_several_cells_contours_and_frames_a_thread(ops, oracle):
    """The scans are one workgroup of 256 threads each.  Two frames of 40 x 72 (320 cells, 3 mask words a row) with
    one-pixel blobs in row 0, row 39 and every third row between: two cells a thread in the cell scan, contours in
    three waves.  300 frames of 3 x 5 with 0, 1 or 2 contours: two frames a thread in the scans over the frames."""
    tall = np.zeros((2, 40, 72), np.uint8)
    for f in range(2):
        for y in sorted(set(range(0, 40, 3)) | {39}):
            tall[f, y, (y + 7 * f) % 5::5] = 1
    tall[1, 39] = 0
    tall[1, 39, 71] = 1
    many = np.zeros((300, 3, 5), np.uint8)
    many[::2, 0, 0] = 1
    many[::3, 2, 4] = 1
    for stack in (tall, many):
        ref = [oracle.find_contours_external_simple(m) for m in stack]
        assert len({len(r) for r in ref}) >= 2
        total, npts = sum(len(r) for r in ref), sum(len(c) for r in ref for c in r)
        rc, out = raw(stack, total, npts)
        assert rc == 0 and out["totals"][:2].tolist() == [total, npts]
        assert out["ncontours"][:len(stack)].tolist() == [len(r) for r in ref]
        assert np.array_equal(out["point_off"][:total + 1], np.arange(total + 1))       # every contour is one point
        assert all(same_lists(g, r) for g, r in zip(lists_of(out, len(stack)), ref))
    assert len(oracle.find_contours_external_simple(tall[0])) > 128


# -------------------------------------------------------------------------------- determinism
def test_two_runs_give_identical_bytes(batch):
    stack, ref = batch
    total, npts = sum(len(r) for r in ref), sum(len(c) for r in ref for c in r)
    a, b = raw(stack, total + 5, npts + 7)[1], raw(stack, total + 5, npts + 7)[1]
    for k in a:
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), k


# -------------------------------------------------------------------------------- consistency
def test_largest_contour_is_one_of_the_list(ops, batch):
    from video.analysis import regions
    stack, _ = batch
    frames = list(stack) + list(G.blob_stack()) + [m for m in G.externality_cases().values()]
    for k, m in enumerate(frames):
        contours, info = ops.find_contours(m, ret_info=True)
        if not contours:
            with pytest.raises(RuntimeError):
                regions.get_contour_from_largest_region(m)
            continue
        best = int(np.argmax(info["area"]))                           # the first maximum
        c, area = regions.get_contour_from_largest_region(m, ret_area=True)
        assert area == info["area"][best], k
        assert np.array_equal(c, np.squeeze(np.asarray(contours[best], np.double))), k


# -------------------------------------------------------------------------------- public layer
def test_regions_find_contours_equals_fixture(fx):
    from video.analysis import regions
    for name, mask in G.all_cases().items():
        ref = G.unflatten(fx["c/%s/points" % name], fx["c/%s/sizes" % name])
        assert same_lists(regions.find_contours(mask), ref), name
    stack = G.batch9()
    got = regions.find_contours(stack.astype(bool))
    for f in range(len(stack)):
        assert same_lists(got[f], G.unflatten(fx["c/batch9/%d/points" % f], fx["c/batch9/%d/sizes" % f])), f


def test_external_contours_equal_fixture(fx):
    from video.analysis import regions
    cases = list(G.ring_cases())
    for key, ring, res in cases:
        got = regions.get_external_contour(ring, res)
        assert got.dtype == np.float64 and np.array_equal(got, fx[key]), key
    batched = regions.get_external_contours([c[1] for c in cases], [c[2] for c in cases])
    for (key, ring, res), got in zip(cases, batched):
        assert np.array_equal(got, fx[key]), key
    same = regions.get_external_contours([c[1] for c in cases[1::2]], 0.5)      # one resolution for all
    for (key, ring, _), got in zip(cases[1::2], same):
        assert np.array_equal(got, regions.get_external_contour(ring, 0.5)), key
    with pytest.raises(ValueError):
        regions.get_external_contour(np.stack([np.arange(1025.0), np.arange(1025.0) ** 2], 1), 1.0)


def test_created_stream_back_to_back(ops, batch):
    from video import _hip
    stack, ref = batch
    L = _hip.lib()
    s = C.c_void_p()
    assert L.va_stream_create(C.byref(s)) == 0
    try:
        first = ops.find_contours(stack, stream=s.value)
        second = ops.find_contours(stack[::-1], moments=True, stream=s.value)
        assert all(same_lists(g, r) for g, r in zip(first, ref))
        assert all(same_lists(g, r) for g, r in zip(second[0], ref[::-1]))
        rc, out = raw(stack, 1000, 4000, stream=s.value)
        assert rc == 0 and all(same_lists(g, r) for g, r in zip(lists_of(out, len(stack)), ref))
    finally:
        L.va_stream_destroy(s.value)


def test_error_table():
    from video import _hip
    from video._hip import DeviceBuffer
    L = _hip.lib()
    n, h, w = 2, 5, 7
    src = DeviceBuffer.from_array(np.ones((n, h, w), np.uint8))
    ws_bytes = L.va_find_contours_workspace_bytes(n, h, w)
    assert ws_bytes >= 256 and L.va_find_contours_workspace_bytes(0, h, w) == 256
    ws, nc, tot, info, off, pts = (DeviceBuffer(ws_bytes), DeviceBuffer(8), DeviceBuffer(16), DeviceBuffer(48 * 4),
                                   DeviceBuffer(8 * 5), DeviceBuffer(8 * 16))
    good = [src.ptr, n, h, w, nc.ptr, tot.ptr, info.ptr, off.ptr, 4, pts.ptr, 16, ws.ptr, ws_bytes, None]
    assert L.va_find_contours(*good) == 0
    assert L.va_stream_sync(None) == 0
    assert tot.download((2,), np.int64).tolist() == [2, 8]
    INVALID = -22
    for pos in (0, 4, 5, 6, 7, 9, 11):                                  # NULL pointers
        bad = list(good)
        bad[pos] = None
        assert L.va_find_contours(*bad) == INVALID, pos
        assert b"va_find_contours" in L.va_last_error()
    for pos, value in ((2, 0), (3, 0), (2, -1), (1, -1), (8, -1), (10, -1), (12, ws_bytes - 1), (12, 0)):
        bad = list(good)
        bad[pos] = value
        assert L.va_find_contours(*bad) == INVALID, (pos, value)
    assert L.va_find_contours(src.ptr, 1, 1 << 15, 1 << 14, nc.ptr, tot.ptr, info.ptr, off.ptr, 4, pts.ptr, 16, ws.ptr,
                              ws_bytes, None) == INVALID               # 2^29 pixels
    empty = list(good)
    empty[1] = 0
    assert L.va_find_contours(*empty) == 0                              # n == 0
    assert L.va_contour_moments_ragged(None, None, 0, 0, None, None) == 0
    assert L.va_contour_moments_ragged(pts.ptr, off.ptr, -1, 0, info.ptr, None) == INVALID
    assert L.va_contour_moments_ragged(None, off.ptr, 1, 0, info.ptr, None) == INVALID
    assert L.va_contour_moments_ragged(pts.ptr, None, 1, 0, info.ptr, None) == INVALID
    assert L.va_contour_moments_ragged(pts.ptr, off.ptr, 1, 0, None, None) == INVALID
    for b in (src, ws, nc, tot, info, off, pts):
        b.free()
