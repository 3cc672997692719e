"""GPU: annotating on the device ("Annotating on the device"): va_draw_contours_u8 /
ops.draw_contours, ops.DeviceContours, FrameEngine's keep=, device planes in ops.compose_layers and
VideoComposer.annotate_frames.  The expected bytes are the closed polylines of the NumPy restatement
tests/composer_checks.py drawn over the contours of the oracle's scanner; everything is exact, so every comparison
is np.array_equal on the bytes."""
import zlib

import numpy as np
import pytest

import composer_checks as K

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (2, 3), (5, 16), (37, 53), (16, 129))
H, W = 37, 53
OK, ERR_RANGE, ERR_INVALID = 0, -34, -22
MAX_COORD = 1 << 20
KINDS = ("empty", "full", "pixel", "bar", "checker", "edges", "noise", "blobs")
# every kind with n = 1; with n = 3 and n = 5 every kind once, and a frame without contours between two with some
STACKS = tuple((k,) for k in KINDS) + (("empty", "full", "pixel"), ("bar", "checker", "edges"),
                                       ("noise", "empty", "blobs"), ("empty", "full", "pixel", "bar", "checker"),
                                       ("edges", "noise", "empty", "blobs", "noise"))


def _rng(*key):
    return np.random.default_rng([zlib.crc32(k.encode()) if isinstance(k, str) else int(k) for k in key])


def _pattern(rng, n, h, w, c):
    """frames pre-filled with a pattern, so that untouched bytes are checked too"""
    return rng.integers(0, 256, (n, h, w) + ((3,) if c == 3 else ()), dtype=np.uint8)


def _mask(rng, kind, h, w):
    m = np.zeros((h, w), np.uint8)
    yy, xx = np.mgrid[:h, :w]
    if kind == "full":
        m[:] = 255
    elif kind == "pixel":
        m[h // 2, w // 2] = 1
    elif kind == "bar":                              # two pixels: a contour of two points (one on a 1-wide frame)
        m[h // 2, w // 2:w // 2 + 2] = 7
    elif kind == "checker":                          # every contour is one point: the set pixels are two apart, as
        m[(yy % 2 == 0) & (xx % 2 == 0)] = 1         # diagonal neighbours would be one 8-connected component
    elif kind == "edges":                            # blobs that touch all four edges
        m[0, :w // 2 + 1] = 1
        m[h - 1, w // 3:] = 1
        m[h // 3:, 0] = 1
        m[:h // 2 + 1, w - 1] = 1
        m[(xx - w // 2) ** 2 + (yy - h // 2) ** 2 <= (min(h, w) // 5) ** 2] = 1
    elif kind == "noise":
        m[rng.random((h, w)) < 0.5] = 200
    elif kind == "blobs":
        m[((xx - w // 4) ** 2 + (yy - h // 3) ** 2 < (h * h) // 20 + 1) | ((abs(xx - 3 * w // 4) < w // 6 + 1) &
                                                                          (abs(yy - 2 * h // 3) < h // 5 + 1))] = 1
    else:
        assert kind == "empty"
    return m


def _colors(c):
    return (0, 255, 137) if c == 1 else ((0, 0, 0), (255, 0, 9), (1, 2, 3))


def _scan(masks):
    from oracle import oracle as O
    return [O.find_contours_external_simple(m) for m in masks]


def _restated(frames, lists, color, frame_map=None):
    """the closed polylines of the restatement; source frame f goes to frame frame_map[f]"""
    commands = [[] for _ in range(len(frames))]
    for f, contours in enumerate(lists):
        t = f if frame_map is None else frame_map[f]
        if t >= 0:
            commands[t] += [("polyline", c, True, color) for c in contours]
    return K.draw(frames, commands)


_CASES = {}


def _cases(h, w, c):
    """[(frames, masks, colour, expected bytes)] of the kernel cases of one shape, computed once"""
    if (h, w, c) not in _CASES:
        out = []
        for i, kinds in enumerate(STACKS):
            rng = _rng("kernel", h, w, c, i)
            masks = np.stack([_mask(rng, k, h, w) for k in kinds])
            frames = _pattern(rng, len(kinds), h, w, c)
            color = _colors(c)[i % 3]
            out.append((frames, masks, color, _restated(frames, _scan(masks), color)))
        for a in out:
            for x in a[:2] + a[3:]:
                x.flags.writeable = False
        _CASES[(h, w, c)] = out
    return _CASES[(h, w, c)]


def _run_cases(h, w, c):
    from video import ops
    got = []
    for frames, masks, color, want in _cases(h, w, c):
        found = ops.find_contours(masks, keep=True)
        try:
            assert found.n == len(masks) and (found.h, found.w) == (h, w) and found.counts.sum() == found.ncontours
            res = ops.draw_contours(frames, found, color)
        finally:
            found.release()
        assert res.dtype == np.uint8 and res.shape == want.shape
        assert np.array_equal(res, want), (len(masks), color, np.argwhere(res != want)[:4])
        got.append(res)
    return got


@pytest.fixture(params=(0xFF, 0xA5), ids=["fill_ff", "fill_a5"])
def hostile(request):
    """the test fill mode around one test, as in tests/test_gpu_hostile_memory.py"""
    from video import _hip, ops
    _hip.lib()
    ops.pool_clear()
    _hip.set_fill_mode(request.param)
    try:
        yield request.param
        found = _hip.check_guards()
    finally:
        _hip.set_fill_mode(-1)
        ops.pool_clear()
        _hip.check_guards()
    assert found == [], found


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("c", (1, 3), ids=("mono", "rgb"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_contours_match_the_restatement(shape, c):
    _run_cases(shape[0], shape[1], c)
    assert any(len(m) == n and m.any() for n in (1, 3, 5) for _, m, _, _ in _cases(shape[0], shape[1], c))
    assert any(col in (0, (0, 0, 0)) for _, _, col, _ in _cases(shape[0], shape[1], c))


def test_the_cases_hold_what_they_are_meant_to():
    lists = {k: _scan([_mask(_rng("meant", k), k, H, W)])[0] for k in KINDS}
    assert lists["empty"] == [] and len(lists["full"]) == 1 and len(lists["full"][0]) == 4
    assert [len(c) for c in lists["pixel"]] == [1] and [len(c) for c in lists["bar"]] == [2]
    assert len(lists["checker"]) == ((H + 1) // 2) * ((W + 1) // 2) and {len(c) for c in lists["checker"]} == {1}
    edge = np.concatenate(lists["edges"]).reshape(-1, 2)
    assert edge[:, 0].min() == 0 and edge[:, 0].max() == W - 1 and edge[:, 1].min() == 0 and edge[:, 1].max() == H - 1
    assert len(lists["noise"]) > 3 and len(lists["blobs"]) == 2


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_kernel_cases_on_dirty_memory(hostile, shape):
    for c in (1, 3):
        first, again = _run_cases(shape[0], shape[1], c), _run_cases(shape[0], shape[1], c)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))


# ------------------------------------------------------------------------------------------------ the existing path
def _three(seed="three"):
    rng = _rng(seed)
    masks = np.stack([_mask(rng, k, H, W) for k in ("noise", "blobs", "empty", "edges")])
    return rng, masks


@pytest.mark.parametrize("c", (1, 3), ids=("mono", "rgb"))
def test_equal_to_draw_with_one_polyline_per_contour(c):
    from video import ops
    rng, masks = _three()
    frames = _pattern(rng, len(masks), H, W, c)
    color = 77 if c == 1 else (9, 200, 31)
    found = ops.find_contours(masks, keep=True)
    try:
        lists = found.download()
        got = ops.draw_contours(frames, found, color)
        dev = ops.DeviceFrames.upload(frames)                   # the resident form: drawn in place, and kept
        same = ops.draw_contours(dev, found, color, keep=True)
        assert same is dev and np.array_equal(dev.download(), got)
        dev.release()
    finally:
        found.release()
    assert np.array_equal(got, ops.draw(frames, [[("polyline", k, True, color) for k in cs] for cs in lists]))
    assert sum(len(cs) for cs in lists) > 10 and (got != frames).any()


def test_download_is_find_contours():
    from video import ops
    _, masks = _three()
    want = ops.find_contours(masks, ret_info=True, moments=True)
    dev = ops.DeviceFrames.upload(masks)
    for source in (masks, dev):                      # masks that are on the device already are not uploaded
        found = ops.find_contours(source, keep=True)
        try:
            assert found.counts.tolist() == [len(cs) for cs in want[0]]
            assert found.npoints == sum(len(k) for cs in want[0] for k in cs)
            for kwargs in (dict(), dict(ret_info=True), dict(moments=True), dict(ret_info=True, moments=True)):
                got = found.download(**kwargs)
                plain = ops.find_contours(masks, **kwargs)
                got, plain = (got, plain) if kwargs else ((got,), (plain,))
                assert len(got) == len(plain) == 1 + len(kwargs)
                for a, b in zip(got, plain):
                    assert len(a) == len(b) == len(masks)
                    for fa, fb in zip(a, b):
                        assert len(fa) == len(fb)
                        for x, y in zip(fa, fb):
                            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
        finally:
            found.release()
    assert np.array_equal(dev.download(), masks)
    dev.release()
    single = ops.find_contours(masks[1])             # the host form of one (h, w) mask: that frame's list
    assert len(single) == len(want[0][1]) and all(np.array_equal(a, b) for a, b in zip(single, want[0][1]))
    with pytest.raises(ValueError):
        rgb = ops.DeviceFrames.upload(np.zeros((1, 4, 4, 3), np.uint8))
        try:
            ops.find_contours(rgb)
        finally:
            rgb.release()


@pytest.mark.parametrize("frame_map,n_out", (((0, 1, 2, 3), 4), ((2, 0, 3, 1), 4), ((1, -1, 0, -1), 2),
                                             ((-1, -1, -1, -1), 1), ((0, 0, 2, 2), 3), (None, 4)))
def test_frame_map(frame_map, n_out):
    from video import ops
    rng, masks = _three("map")
    frames = _pattern(rng, n_out, H, W, 3)
    found = ops.find_contours(masks, keep=True)
    try:
        got = ops.draw_contours(frames, found, (0, 250, 3), frame_map=frame_map)
    finally:
        found.release()
    assert np.array_equal(got, _restated(frames, _scan(masks), (0, 250, 3), frame_map))


# ------------------------------------------------------------------------------------------------ the C ABI
def _tables():
    """a find_contours result as host arrays: (info, point_off, points)"""
    from video import ops
    _, masks = _three("abi")
    found = ops.find_contours(masks, keep=True)
    try:
        info = found.info.download((found.ncontours,), ops.CONTOUR_INFO_DTYPE)
        off = found.point_off.download((found.ncontours + 1,), np.int64)
        points = found.points.download((found.npoints, 2), np.int32)
    finally:
        found.release()
    assert off[0] == 0 and off[-1] == len(points) and (np.diff(off) == info["npoints"]).all()
    return len(masks), info, off, points


def _survivors(frames, info, off, points, ncontours, npoints, fmap, n_src, color):
    """the refusal rules of the section, restated: (expected bytes, expected status)"""
    out, status = frames.copy(), OK
    h, w = frames.shape[1:3]
    for s in range(ncontours):
        lo, hi, f = int(off[s]), int(off[s + 1]), int(info["frame"][s])
        if not 0 <= lo <= hi <= npoints or not 0 <= f < n_src:
            status = ERR_RANGE
            continue
        t = f if fmap is None else int(fmap[f])
        if t == -1 and fmap is not None:
            continue
        if not 0 <= t < len(frames):
            status = ERR_RANGE
            continue
        for p in range(lo, hi):
            q = lo if p + 1 == hi else p + 1
            ends = [int(v) for v in (*points[p], *points[q])]
            if max(abs(v) for v in ends) > MAX_COORD:
                status = ERR_RANGE
                continue
            for x, y in K.line_pixels(w, h, *ends):
                out[t, y, x] = color
    return out, status


def _abi_call(frames, info, off, points, ncontours, npoints, fmap, n_src, color, c):
    """va_draw_contours_u8 on private buffers (guarded in the fill mode): (bytes, status)"""
    from video import _hip
    L = _hip.lib()
    bufs = [_hip.DeviceBuffer.from_array(a) if a is not None and a.size else None
            for a in (frames, info, off, points, None if fmap is None else np.asarray(fmap, np.int32))]
    st = _hip.DeviceBuffer.from_array(np.array([12345], np.int32))
    ptr = [None if b is None else b.ptr for b in bufs]
    packed = color if c == 1 else color[0] | color[1] << 8 | color[2] << 16
    try:
        _hip.check(L.va_draw_contours_u8(ptr[0], len(frames), frames.shape[1], frames.shape[2], c, ptr[1], ptr[2],
                                         ncontours, ptr[3], npoints, ptr[4], n_src, packed, st.ptr, None))
        return bufs[0].download(frames.shape, np.uint8), int(st.download((1,), np.int32)[0])
    finally:
        for b in bufs + [st]:
            if b is not None:
                b.free()


def _longest(info):
    """the slot with the most points among 1 .. k - 4 (the prefix case cuts into the last three)"""
    return 1 + int(np.argmax(info["npoints"][1:len(info) - 3]))


def _damaged(n_src, info, off, points):
    """name -> (info, off, points, ncontours, npoints, frame_map, n_out); the offsets are damaged in their last
    entry, where the slots' ranges stay disjoint and the slot of every point stays defined"""
    k, npts = len(info), len(points)
    mid = _longest(info)
    cases = {}

    def put(name, info=info, off=off, points=points, ncontours=k, npoints=npts, fmap=None, n_out=n_src):
        cases[name] = (info, off, points, ncontours, npoints, fmap, n_out)

    for name, value in (("frame_minus_one", -1), ("frame_n_src", n_src)):
        bad = info.copy()
        bad["frame"][mid] = value
        put(name, info=bad)
    put("map_n_out", fmap=[0, n_src, 1, 2])           # the contours of source frame 1 have no target
    put("n_out_too_small", n_out=n_src - 1)           # the identity leads behind the stack
    for name, value in (("off_decreasing", off[k - 1] - 1), ("off_beyond", npts + 3)):
        bad = off.copy()
        bad[k] = value
        put(name, off=bad)
    bad = points.copy()
    bad[off[mid] + 1, 0] = MAX_COORD + 1              # two segments end there
    put("coordinate", points=bad)
    bad = points.copy()
    bad[off[1], 1] = -MAX_COORD - 1
    put("coordinate_negative", points=bad)
    put("prefix", ncontours=k - 2, npoints=int(off[k - 3]) + 1)         # the capacity prefix: slot k - 3 lost its points
    return cases


@pytest.mark.parametrize("c", (1, 3), ids=("mono", "rgb"))
def test_abi_with_damaged_tables(hostile, c):
    n_src, info, off, points = _tables()
    assert len(info) >= 8 and info["npoints"][_longest(info)] >= 3 and info["npoints"][len(info) - 3] >= 2
    color = 201 if c == 1 else (5, 0, 250)
    rng = _rng("damaged", c)
    sound = None
    for name, (i, o, p, k, npts, fmap, n_out) in _damaged(n_src, info, off, points).items():
        frames = _pattern(rng, n_out, H, W, c)
        want, status = _survivors(frames, i, o, p, k, npts, fmap, n_src, color)
        assert status == ERR_RANGE, name
        got, st = _abi_call(frames, i, o, p, k, npts, fmap, n_src, color, c)
        assert st == ERR_RANGE, name
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:4])
        if sound is None:                             # the undamaged tables: VA_OK, and more is drawn
            sound, st = _abi_call(frames, info, off, points, len(info), len(points), None, n_src, color, c)
            assert st == OK and np.array_equal(sound, _survivors(frames, info, off, points, len(info), len(points),
                                                                 None, n_src, color)[0])
            assert (sound != frames).sum() > (got != frames).sum() > 0
    # offsets damaged in the middle of the table: refused, and nothing outside the buffers is touched (the guards)
    for value in (-1, off[-1] + 5, off[len(info) // 2 - 1] - 1, off[len(info) // 2 + 1] + 1):
        bad = off.copy()
        bad[len(info) // 2] = value
        frames = _pattern(rng, n_src, H, W, c)
        assert _abi_call(frames, info, bad, points, len(info), len(points), None, n_src, color, c)[1] == ERR_RANGE


def test_abi_status_and_invalid_arguments():
    from video import _hip
    L = _hip.lib()
    n_src, info, off, points = _tables()
    frames = _pattern(_rng("invalid"), n_src, H, W, 1)
    got, st = _abi_call(frames, None, None, None, 0, 0, None, 0, 9, 1)          # ncontours == 0 writes VA_OK
    assert st == OK and np.array_equal(got, frames)
    got, st = _abi_call(frames, info, off, points, 0, len(points), None, n_src, 9, 1)
    assert st == OK and np.array_equal(got, frames)
    bufs = [_hip.DeviceBuffer.from_array(a) for a in (frames, info, off, points)]
    st = _hip.DeviceBuffer.from_array(np.array([7], np.int32))
    f, i, o, p = (b.ptr for b in bufs)
    k, m = len(info), len(points)
    fn = L.va_draw_contours_u8
    for args in ((f, n_src, H, W, 2, i, o, k, p, m, None, n_src, 1, st.ptr, None),        # channels
                 (f, -1, H, W, 1, i, o, k, p, m, None, n_src, 1, st.ptr, None),           # negative counts
                 (f, n_src, H, W, 1, i, o, -1, p, m, None, n_src, 1, st.ptr, None),
                 (f, n_src, H, W, 1, i, o, k, p, -1, None, n_src, 1, st.ptr, None),
                 (f, n_src, H, W, 1, i, o, k, p, m, None, -1, 1, st.ptr, None),
                 (f, n_src, H, W, 1, i, o, k, p, m, None, n_src, 1, None, None),          # NULL where data is required
                 (None, n_src, H, W, 1, i, o, k, p, m, None, n_src, 1, st.ptr, None),
                 (f, n_src, H, W, 1, None, o, k, p, m, None, n_src, 1, st.ptr, None),
                 (f, n_src, H, W, 1, i, None, k, p, m, None, n_src, 1, st.ptr, None),
                 (f, n_src, H, W, 1, i, o, k, None, m, None, n_src, 1, st.ptr, None),
                 (f, n_src, 1 << 15, 1 << 14, 1, i, o, k, p, m, None, n_src, 1, st.ptr, None)):   # 2^29 pixels
        assert fn(*args) == ERR_INVALID, args
    assert int(st.download((1,), np.int32)[0]) == 7 and np.array_equal(bufs[0].download(frames.shape, np.uint8), frames)
    for b in bufs + [st]:
        b.free()


def test_draw_contours_raises_for_a_refused_contour():
    from video import ops
    _, masks = _three("refused")
    frames = _pattern(_rng("refused"), len(masks), H, W, 1)
    found = ops.find_contours(masks, keep=True)
    try:
        found.n -= 1                                 # behind the host's checks: the last frame's contours are now
        with pytest.raises(RuntimeError, match="status -34"):                   # outside 0 .. n_src - 1
            ops.draw_contours(frames, found, 5, frame_map=[0, 1, 2])
        found.n += 1                                 # the pool and the library are fine afterwards
        assert np.array_equal(ops.draw_contours(frames, found, 5), _restated(frames, _scan(masks), 5))
    finally:
        found.release()


# ------------------------------------------------------------------------------------------------ the engine
def test_engine_keeps_outputs_on_the_device():
    from video import ops
    from video.engine import FrameEngine
    n, h, w = 8, 48, 64
    rng = _rng("engine")
    yy, xx = np.mgrid[:h, :w]
    clip = np.stack([np.where((xx - 12 - 4 * t) ** 2 + (yy - 20) ** 2 < 60, 200, 40) + rng.integers(0, 20, (h, w))
                     for t in range(n)]).astype(np.uint8)
    eng = FrameEngine(size=(w, h), max_batch=n, sigma=1.5, thresh=100, morphology=(("dilate", "rect", 3),))
    try:
        # (a kept output is not downloaded, so the downloaded mask comes from a run of its own: the engine has no
        # background model, and its runs on the same frames are the same computation)
        plain = eng.run(clip, want=("mask", "filtered"))
        out = eng.run(clip, want=(), keep=("mask",))
        kept = out["mask"]
        assert isinstance(kept, ops.DeviceFrames) and kept.shape == (n, h, w) and set(out) == {"mask"}
        assert np.array_equal(kept.download(), plain["mask"]) and plain["mask"].any() and not plain["mask"].all()
        other = eng.run(255 - clip, want=("mask",))                 # the engine's next run does not change it
        assert not np.array_equal(other["mask"], plain["mask"])
        assert np.array_equal(kept.download(), plain["mask"])
        dev = ops.DeviceFrames.upload(clip)
        both = eng.run_frames(dev, want=(), keep=("mask", "filtered"))
        assert sorted(both) == ["filtered", "mask"]
        assert np.array_equal(both["mask"].download(), plain["mask"])
        assert np.array_equal(both["filtered"].download(), plain["filtered"])
        found = ops.find_contours(both["mask"], keep=True)          # the hand-over: no mask crosses to the host
        assert found.counts.tolist() == [len(cs) for cs in ops.find_contours(plain["mask"])]
        for held in (found, kept, dev, both["mask"], both["filtered"]):
            held.release()
        for keep in (("labels",), ("mask", "counts"), "stats"):
            with pytest.raises(ValueError):
                eng.run(clip, keep=keep)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ device planes
@pytest.mark.parametrize("c", (1, 3), ids=("mono", "rgb"))
def test_compose_layers_with_device_planes(c):
    from video import ops
    n = 3
    rng = _rng("planes", c)
    frames = _pattern(rng, n, H, W, c)
    masks = (rng.random((n, H, W)) < 0.5).astype(np.uint8) * 3
    images = _pattern(rng, 2, H, W, c)
    mdev, idev = ops.DeviceFrames.upload(masks), ops.DeviceFrames.upload(images)
    channel = "g" if c == 3 else "all"
    for host, device in (([[("highlight", masks[f], channel, 128)] for f in range(n)],
                          [[("highlight", (mdev, f), channel, 128)] for f in range(n)]),
                         ([[("highlight", masks[f], "all", 60), ("blend", images[f % 2], 0.3, masks[(f + 1) % n])]
                           for f in range(n)],
                          [[("highlight", (mdev, f), "all", 60), ("blend", (idev, f % 2), 0.3, (mdev, (f + 1) % n))]
                           for f in range(n)]),
                         ([[("add", images[1], None)], [], [("blend", images[0], 0.5, masks[2])]],
                          [[("add", (idev, 1), None)], [], [("blend", (idev, 0), 0.5, (mdev, 2))]])):
        want = ops.compose_layers(frames, host)
        assert np.array_equal(want, K.compose_layers(frames, host))
        assert np.array_equal(ops.compose_layers(frames, device), want)
    # the planes are the caller's, unchanged
    assert np.array_equal(mdev.download(), masks) and np.array_equal(idev.download(), images)
    with pytest.raises(ValueError):
        ops.compose_layers(frames, [[("highlight", (mdev, 0), None, 5), ("highlight", masks[1], None, 5)], [], []])
    mdev.release()
    idev.release()


# ------------------------------------------------------------------------------------------------ the composer
N_CLIP, BATCH = 40, 16


def _clip():
    rng = _rng("composer clip")
    frames = rng.integers(0, 256, (N_CLIP, H, W), dtype=np.uint8)
    yy, xx = np.mgrid[:H, :W]
    masks = np.stack([((xx - 10 - t % 30) ** 2 + (yy - 14) ** 2 < 40) | ((xx - 40) ** 2 + (yy - 30 + t % 7) ** 2 < 20) |
                      (rng.random((H, W)) < 0.02) for t in range(N_CLIP)]).astype(np.uint8)
    return frames, masks


_LOOPS = {}


def _per_frame(period, sink=None):
    """the per-frame loop of the issue through the composer itself; into sink None its frames are computed once"""
    from video import ops
    from video.io.composer import VideoComposer
    if sink is None and period in _LOOPS:
        return _LOOPS[period]
    frames, masks = _clip()
    lists = ops.find_contours(masks)
    vc = VideoComposer(sink, (W, H), 25, True, output_period=period, batch=BATCH)
    for i in range(N_CLIP):
        vc.set_frame(frames[i])
        vc.highlight_mask(masks[i], "g", 100)
        vc.add_contour(lists[i], "r")
    vc.close()
    if sink is None:
        _LOOPS[period] = vc.frames
        _LOOPS[period].flags.writeable = False
        return _LOOPS[period]


def _batched(vc, device_masks, given_contours):
    """the clip through annotate_frames in batches of 16 (16, 16 and 8 frames)"""
    from video import ops
    frames, masks = _clip()
    for start in range(0, N_CLIP, BATCH):
        f, m = frames[start:start + BATCH], masks[start:start + BATCH]
        held = []
        try:
            if device_masks:
                held.append(ops.DeviceFrames.upload(f))
                held.append(ops.DeviceFrames.upload(m))
                f, m = held
            contours = True
            if given_contours:
                contours = ops.find_contours(m if device_masks else masks[start:start + BATCH], keep=True)
                held.append(contours)
            vc.annotate_frames(f, m, "g", 100, contours=contours, color="r")
            assert vc.frame is None
            if device_masks:                         # what is handed in stays as it was
                assert np.array_equal(held[0].download(), frames[start:start + BATCH])
                assert np.array_equal(held[1].download(), masks[start:start + BATCH])
        finally:
            for x in held:
                x.release()


@pytest.mark.parametrize("period", (1, 3))
@pytest.mark.parametrize("given_contours", (False, True), ids=("contours_true", "device_contours"))
@pytest.mark.parametrize("device_masks", (False, True), ids=("host_masks", "device_masks"))
def test_annotate_frames_is_the_per_frame_loop(device_masks, given_contours, period):
    from video.io.composer import VideoComposer
    vc = VideoComposer(None, (W, H), 25, True, output_period=period, batch=BATCH)
    _batched(vc, device_masks, given_contours)
    vc.close()
    want = _per_frame(period)
    assert vc.frames.shape == want.shape == (len(range(0, N_CLIP, period)), H, W, 3)
    assert vc.frames_written == len(want) and vc.next_frame == N_CLIP - 1
    assert np.array_equal(vc.frames, want), np.argwhere(vc.frames != want)[:4]
    assert (want != np.repeat(_clip()[0][::period, :, :, None], 3, axis=3)).any()


@pytest.mark.parametrize("period", (1, 3))
def test_annotate_frames_into_a_stack_sink(period):
    from video import ops
    from video.io.composer import VideoComposer
    got = []

    class Sink(object):
        def write_frames(self, stack):
            assert isinstance(stack, ops.DeviceFrames)
            got.append(stack.download())
    vc = VideoComposer(Sink(), (W, H), 25, True, output_period=period, batch=BATCH)
    _batched(vc, True, True)
    vc.close()
    assert len(got) == 3 and np.array_equal(np.concatenate(got), _per_frame(period))
    assert vc.frames_written == len(_per_frame(period))


def test_annotate_frames_into_a_motion_jpeg_file(tmp_path):
    from video.io.composer import VideoComposer
    a, b = str(tmp_path / "batched.avi"), str(tmp_path / "per_frame.avi")
    vc = VideoComposer(a, (W, H), 25, True, batch=BATCH)
    _batched(vc, True, False)
    vc.close()
    _per_frame(1, sink=b)
    data = open(a, "rb").read()
    assert len(data) > 10000 and data == open(b, "rb").read()


def test_per_frame_calls_mix_with_batches():
    from video import ops
    from video.io.composer import VideoComposer
    frames, masks = _clip()
    lists = ops.find_contours(masks[:12])
    mixed, loop = (VideoComposer(None, (W, H), 25, False, batch=4) for _ in range(2))
    for vc in (mixed, loop):
        for i in range(3):                           # pending per-frame work: flushed before the batch
            vc.set_frame(frames[i])
            vc.add_circle((5 + i, 9), 3, "w", thickness=1)
    mixed.annotate_frames(frames[3:9], masks[3:9], "all", 50, contours=True, color=(0.5, 0.5, 0.5))
    for i in range(3, 9):
        loop.set_frame(frames[i])
        loop.highlight_mask(masks[i], "all", 50)
        loop.add_contour(lists[i], (0.5, 0.5, 0.5))
    for vc in (mixed, loop):
        for i in range(9, 12):
            vc.set_frame(frames[i])
            vc.add_contour(masks[i], "w")
        vc.close()
    assert mixed.frames.shape == (12, H, W) and np.array_equal(mixed.frames, loop.frames)


def test_composer_clip_on_dirty_memory(hostile):
    from video.io.composer import VideoComposer
    results = []
    for run in (1, 2):
        vc = VideoComposer(None, (W, H), 25, True, output_period=3, batch=BATCH)
        _batched(vc, True, run == 1)                 # a DeviceContours handed in, then contours=True
        vc.close()
        results.append(vc.frames)
    assert np.array_equal(results[0], _per_frame(3)) and results[0].tobytes() == results[1].tobytes()
