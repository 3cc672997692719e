"""GPU: ops.compose_layers, ops.draw and video.io.composer against the NumPy restatement tests/composer_checks.py
("Composer").  All arithmetic is exact, so every comparison is np.array_equal on the bytes."""
import zlib

import numpy as np
import pytest

import composer_checks as K

pytestmark = pytest.mark.gpu

LAYER_SHAPES = ((1, 1), (2, 3), (5, 16), (37, 53), (16, 129))     # the vector body, the tail, rows below 16 pixels
H, W = 37, 53


def _rng(*key):
    return np.random.default_rng([zlib.crc32(k.encode()) if isinstance(k, str) else int(k) for k in key])


def _frames(rng, n, h, w, c):
    return rng.integers(0, 256, (n, h, w) + ((3,) if c == 3 else ()), dtype=np.uint8)


def _mask(rng, h, w, kind="random"):
    if kind == "zeros":
        return np.zeros((h, w), bool)
    if kind == "ones":
        return np.ones((h, w), np.uint8) * 7            # a uint8 mask: non-zero is what counts
    return rng.random((h, w)) < 0.5


def _image(rng, h, w, c):
    return rng.integers(0, 256, (h, w) + ((3,) if c == 3 else ()), dtype=np.uint8)


def _layer_lists(rng, n, h, w, c, which):
    """the layer lists of the issue's cases for n frames of c output channels"""
    def one(kind, f):
        mask = _mask(rng, h, w, ("random", "zeros", "ones")[f % 3])
        if kind == "highlight":
            channel = ("all", None, "g", 2)[f % 4] if c == 3 else ("all", None)[f % 2]
            return ("highlight", mask, channel, (0, 128, 255)[f % 3])
        if kind == "add":
            return ("add", _image(rng, h, w, (1, c)[f % 2]), (None, mask)[f % 2])
        return ("blend", _image(rng, h, w, (c, 1)[f % 2]), (0, 1, 0.5, 0.3)[f % 4], (mask, None)[f % 2])
    if which in ("highlight", "add", "blend"):
        return [[one(which, f)] for f in range(n)]
    if which == "mixed6":
        return [[one(k, f + i) for i, k in enumerate(("blend", "highlight", "add", "highlight", "blend", "add"))]
                for f in range(n)]
    assert which == "gap"                            # a frame with no layers between frames with some
    return [[one("blend", f), one("highlight", f + 1)] if f != 1 else [] for f in range(n)]


# ------------------------------------------------------------------------------------------------ layers
@pytest.mark.parametrize("shape", LAYER_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("chan", ((1, 1), (1, 3), (3, 3)), ids=lambda c: "%dto%d" % c)
@pytest.mark.parametrize("n", (1, 3))
def test_layers_match_the_restatement(shape, chan, n):
    from video import ops
    (h, w), (c_src, c) = shape, chan
    for which in ("highlight", "add", "blend", "mixed6", "gap"):
        rng = _rng(h, w, c_src, c, n, which)
        frames = _frames(rng, n, h, w, c_src)
        layers = _layer_lists(rng, n, h, w, c, which)
        got = ops.compose_layers(frames, layers, color=(c == 3))
        want = K.compose_layers(frames, layers, color=(c == 3))
        assert got.dtype == np.uint8 and got.shape == want.shape
        assert np.array_equal(got, want), (which, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("weight", (0.5, 0.3))
def test_blend_of_every_byte_pair(weight):
    """all (v, u) as one 256 x 256 frame: every tie and both saturation ends"""
    from video import ops
    v, u = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    got = ops.compose_layers(v[None], [[("blend", u, weight, None)]])[0]
    assert np.array_equal(got, K.blend_values(v, u, weight))
    if weight == 0.5:                                # ties go to the even neighbour
        assert got[1, 0] == 0 and got[3, 0] == 2 and got[255, 254] == 254 and got[255, 255] == 255


def test_layers_host_errors():
    from video import ops
    mono, rgb = np.zeros((1, 4, 5), np.uint8), np.zeros((1, 4, 5, 3), np.uint8)
    m, im, im3 = np.ones((4, 5), bool), np.zeros((4, 5), np.uint8), np.zeros((4, 5, 3), np.uint8)
    for frames, layers, color in ((mono, [[("highlight", m, "r", 10)]], None), (rgb, [[("highlight", m, "x", 10)]], None),
                                  (mono, [[("highlight", m, "all", 256)]], None), (mono, [[("add", im3, None)]], None),
                                  (mono, [[("add", im[:3], None)]], None), (mono, [[("blend", im, 0.5, m[:, :4])]], None),
                                  (rgb, [[]], False), (mono, [[], []], None), (mono, [[("shade", im)]], None)):
        with pytest.raises(ValueError):
            ops.compose_layers(frames, layers, color=color)


# ------------------------------------------------------------------------------------------------ drawing
def _octant_segments():
    c = (26, 18)
    ends = [(40, 18), (40, 25), (38, 30), (31, 32), (26, 33), (20, 32), (12, 30), (10, 24), (9, 18), (11, 12),
            (14, 5), (21, 3), (26, 2), (30, 4), (38, 6), (41, 12)]
    return [[c, e] for e in ends] + [[(7, 7), (7, 7)]]


def _clipped_segments():
    return [[(-10, 5), (20, 30)], [(20, 30), (80, 8)], [(-7, -3), (70, 50)], [(-20, 10), (-3, 30)], [(5, -40), (60, -2)],
            [(60, 20), (10, 90)], [(-5, 36), (58, 37)], [(52, -9), (53, 44)], [(-1000000, -999999), (1000000, 1048576)]]


def _circle_cmds(col):
    cmds = []
    for i, r in enumerate((0, 1, 2, 3, 4, 5, 6, 20)):
        for center in ((20 + i, 15 + i), (0, 10), (52, 36), (-4, 18), (26, 36 + r), (60, -3)):
            for filled in (True, False):
                cmds.append(("circle", center, r, filled, col(len(cmds))))
    cmds.append(("circle", (10, 10), -1, True, col(0)))
    return cmds


def _draw_cases(c):
    def col(i):
        v = 1 + (37 * i) % 255
        return v if c == 1 else (v, 255 - v, (v * 7) % 256)
    rng = _rng("draw", c)
    long_line = np.cumsum(rng.integers(-4, 5, (601, 2)), axis=0) + (26, 18)
    same = [("circle", tuple(rng.integers(-3, 56, 2)), int(rng.integers(0, 4)), bool(i % 2), col(3)) for i in range(300)]
    cases = {
        "octants": [("polyline", s, False, col(i)) for i, s in enumerate(_octant_segments())],
        "clipped": [("polyline", s, bool(i % 2), col(i)) for i, s in enumerate(_clipped_segments())],
        "long": [("polyline", long_line, True, col(1))],
        "circles": _circle_cmds(col),
        "order_ab": [("circle", (20, 18), 9, True, col(1)), ("polyline", [(5, 18), (45, 19)], False, col(2))],
        "order_ba": [("polyline", [(5, 18), (45, 19)], False, col(2)), ("circle", (20, 18), 9, True, col(1))],
        "run": same + [("circle", (26, 18), 12, True, col(9))],
        "tiny": [("polyline", np.zeros((0, 2), np.int32), True, col(1)), ("polyline", [(3, 3)], False, col(2)),
                 ("polyline", [(5, 5)], True, col(3)), ("polyline", [(8, 8), (12, 9)], True, col(4))],
        "none": [],
    }
    return cases


@pytest.mark.parametrize("c", (1, 3), ids=("mono", "rgb"))
@pytest.mark.parametrize("shape", ((H, W), (1, 1)), ids=lambda s: "%dx%d" % s)
def test_draw_matches_the_restatement(c, shape):
    """every case is one frame of a stack, so the launch also mixes frames with and without commands"""
    from video import ops
    h, w = shape
    cases = _draw_cases(c)
    frames = _frames(_rng("frames", c, h), len(cases), h, w, c)
    commands = list(cases.values())
    got = ops.draw(frames, commands)
    want = K.draw(frames, commands)
    for i, name in enumerate(cases):
        assert np.array_equal(got[i], want[i]), (name, np.argwhere(got[i] != want[i])[:4])
    assert np.array_equal(got[-1], frames[-1])
    assert not np.array_equal(want[list(cases).index("order_ab")], want[list(cases).index("order_ba")]) or h == 1
    again = ops.draw(frames, commands)               # determinism: two runs write identical bytes
    assert got.tobytes() == again.tobytes()


def test_draw_takes_find_contours_output_as_it_is():
    from video import ops
    yy, xx = np.mgrid[:H, :W]
    masks = np.stack([((xx - 20) ** 2 + (yy - 15) ** 2 < 90) | ((xx - 40) ** 2 + (yy - 28) ** 2 < 50),
                      (abs(xx - 25) < 9) & (abs(yy - 20) < 6)]).astype(np.uint8)
    frames = _frames(_rng("contours"), 2, H, W, 3)
    contours = ops.find_contours(masks)
    assert all(c.shape[1:] == (1, 2) and c.dtype == np.int32 for cs in contours for c in cs)
    commands = [[("polyline", c, True, (255, 0, 9)) for c in cs] for cs in contours]
    got = ops.draw(frames, commands)
    assert np.array_equal(got, K.draw(frames, commands))
    assert (got != frames).any(axis=3).sum() >= sum(len(c) for cs in contours for c in cs)


def test_draw_host_errors():
    from video import ops
    mono = np.zeros((1, 4, 5), np.uint8)
    big = (1 << 20) + 1
    for cmds in ([("polyline", [(0, big)], True, 1)], [("circle", (0, 0), big, True, 1)], [("circle", (-big, 0), 1, True, 1)],
                 [("polyline", [(0, 0)], True, 256)], [("polyline", [(0, 0)], True, (1, 2, 3))], [("square", 1)]):
        with pytest.raises(ValueError):
            ops.draw(mono, [cmds])
    with pytest.raises(TypeError):
        ops.draw(mono, [[("polyline", [(0.5, 1.0)], True, 1)]])
    with pytest.raises(ValueError):
        ops.draw(mono, [[], []])


def test_device_refuses_one_frame_and_draws_the_others():
    """through the C ABI: a point range outside the buffer, a coordinate beyond the limit and an unknown kind give
    VA_ERR_RANGE for their frames, which stay untouched, while the other frames are drawn"""
    from video import _hip, ops
    L = _hip.lib()
    n = 5
    frames = _frames(_rng("refuse"), n, H, W, 1)
    good = [("polyline", [(2, 3), (40, 30), (10, 33)], True, 200), ("circle", (30, 12), 6, True, 90)]
    table, off, points = ops._draw_tables([good] * n, n, 1, "test")
    points = points.copy()
    per = len(good)
    table["count"][1 * per] = len(points) + 1                   # frame 1: the range leaves the buffer
    points[table["first"][2 * per] + 1, 0] = (1 << 20) + 1      # frame 2: a coordinate beyond the limit
    table["kind"][3 * per + 1] = 7                              # frame 3: an unknown kind
    bufs = [_hip.DeviceBuffer.from_array(a) for a in (frames, table, off, points)]
    st = _hip.DeviceBuffer(n * 4)
    _hip.check(L.va_draw_u8(bufs[0].ptr, n, H, W, 1, bufs[1].ptr, bufs[2].ptr, len(table), bufs[3].ptr, len(points),
                            st.ptr, None))
    status = st.download((n,), np.int32)
    got = bufs[0].download(frames.shape, np.uint8)
    assert status.tolist() == [0, -34, -34, -34, 0]
    want = K.draw(frames, [good, [], [], [], good])
    assert np.array_equal(got, want)
    # bad scalars are VA_ERR_INVALID; empty tables launch nothing
    assert L.va_draw_u8(bufs[0].ptr, n, H, W, 2, bufs[1].ptr, bufs[2].ptr, len(table), bufs[3].ptr, len(points),
                        st.ptr, None) == -22
    assert L.va_draw_u8(bufs[0].ptr, -1, H, W, 1, bufs[1].ptr, bufs[2].ptr, len(table), bufs[3].ptr, len(points),
                        st.ptr, None) == -22
    assert L.va_draw_u8(None, 0, H, W, 1, None, None, 0, None, 0, None, None) == 0
    assert L.va_compose_layers_u8(bufs[0].ptr, 3, bufs[0].ptr, n, H, W, 1, None, bufs[2].ptr, 0, None, 0, None, 0,
                                  None) == -22
    assert L.va_compose_layers_u8(bufs[0].ptr, 1, bufs[0].ptr, n, H, W, 3, None, bufs[2].ptr, 0, None, 0, None, 0,
                                  None) == -22                   # 1 -> 3 channels needs a distinct destination
    assert L.va_compose_layers_u8(None, 1, None, 0, H, W, 1, None, None, 0, None, 0, None, 0, None) == 0
    for b in bufs + [st]:
        b.free()


def test_draw_raises_for_a_frame_the_device_refused(monkeypatch):
    """the status-to-exception path of ops.draw: the host's tables are corrupted behind its checks"""
    from video import ops
    tables = ops._draw_tables

    def corrupted(commands, n, c, what):
        table, off, points = tables(commands, n, c, what)
        table["kind"][off[1]] = 7                               # the first command of frame 1
        return table, off, points
    monkeypatch.setattr(ops, "_draw_tables", corrupted)
    frames = _frames(_rng("runtime"), 3, H, W, 1)
    with pytest.raises(RuntimeError, match="refused frame 1"):
        ops.draw(frames, [[("circle", (5, 5), 2, True, 9)]] * 3)
    monkeypatch.undo()
    assert np.array_equal(ops.draw(frames, [[]] * 3), frames)   # the pool and the library are fine afterwards
    got = ops.draw(frames, [[("circle", (5, 5), 2, True, 9)]] * 3)
    assert np.array_equal(got, K.draw(frames, [[("circle", (5, 5), 2, True, 9)]] * 3))


def test_compose_skips_layers_outside_their_buffers():
    """through the C ABI: a layer whose image or mask offset leaves the buffer is not applied, the others are"""
    from video import _hip, ops
    L = _hip.lib()
    rng = _rng("outside")
    frames = _frames(rng, 2, H, W, 1)
    im, m = _image(rng, H, W, 1), _mask(rng, H, W)
    layers = [[("add", im, m), ("highlight", m, None, 50)], [("blend", im, 0.3, None)]]
    table, off, images, masks = ops._compose_tables(layers, 2, H, W, 1, "test")
    table["image_off"][0] = 16                                  # the image would end 16 bytes behind the buffer
    table["mask_off"][1] = len(masks)
    bufs = [_hip.DeviceBuffer.from_array(a) for a in (frames, table, off, images, masks)]
    _hip.check(L.va_compose_layers_u8(bufs[0].ptr, 1, bufs[0].ptr, 2, H, W, 1, bufs[1].ptr, bufs[2].ptr, len(table),
                                      bufs[3].ptr, len(images), bufs[4].ptr, len(masks), None))
    got = bufs[0].download(frames.shape, np.uint8)
    assert np.array_equal(got, K.compose_layers(frames, [[], layers[1]]))
    for b in bufs:
        b.free()


# ------------------------------------------------------------------------------------------------ the composer
def _blob_masks(n, h, w):
    yy, xx = np.mgrid[:h, :w]
    return np.stack([((xx - 14 - t) ** 2 + (yy - 16) ** 2 < 60) | ((xx - 44) ** 2 + (yy - 30 + t % 7) ** 2 < 30)
                     for t in range(n)])


def _tracker_calls(target, t, frame, mask, background):
    """a realistic sequence of one frame of a tracker"""
    target.set_frame(frame)
    target.highlight_mask(mask, "g", 128)
    target.blend_image(background, 0.3)
    target.add_contour(mask.astype(np.uint8), "r")
    target.add_line([(4 + t % 5, 6), (30, 40), (60, 20 + t % 9), (0, 0), (50, 44), (58, 46)], "b", is_closed=False)
    target.add_rectangle((8 + t % 11, 9, 30, 20), "y")
    target.add_points([(12, 12 + t % 13), (33.5, 20.25), (63, 47)], radius=1 + t % 2, color="w")


@pytest.mark.parametrize("zoom", (1, 2))
def test_composer_clip(zoom):
    from video import ops
    from video.io.composer import VideoComposer, get_color
    n, h, w = 120, 48, 64                            # output_period 3: 40 output frames, two full flushes and a tail
    rng = _rng("clip")
    clip = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    masks, background = _blob_masks(n, h, w), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    vc = VideoComposer(None, (w, h), 25, True, output_period=3, zoom_factor=zoom, batch=16)
    rp = K.Replay((w, h), True, output_period=3, zoom_factor=zoom, resize=ops.resize,
                  find_contours=ops.find_contours, get_color=get_color)
    written = []
    for t in range(n):
        for target in (vc, rp):
            _tracker_calls(target, t, clip[t], masks[t], background)
        written.append(vc.frames_written)
    vc.close()
    want = rp.close()
    assert vc.frames.shape == (40, h // zoom, w // zoom, 3) and vc.frames_written == 40
    assert np.array_equal(vc.frames, want)
    assert sorted(set(written)) == [0, 16, 32]       # two full flushes before close()


def test_composer_listener_on_a_video_memory():
    from video.io.base import VideoFilterBase
    from video.io.composer import VideoComposerListener, get_color
    from video.io.memory import VideoMemory
    rng = _rng("listener")
    # (listeners see the frames that pass a video's _process_frame: a filter over the memory, not its raw get_frame)
    video = VideoFilterBase(VideoMemory(rng.integers(0, 256, (5, 24, 32), dtype=np.uint8)))
    vc = VideoComposerListener(None, video, batch=2)
    rp = K.Replay((32, 24), False, get_color=get_color)
    for t, frame in enumerate(video):
        rp.set_frame(frame)
        for target in (vc, rp):
            target.add_circle((5 + 3 * t, 9), 3, "w", thickness=1)
            target.add_rectangle((2, 3, 20, 10 + t), (0.5, 0.5, 0.5))
    assert np.array_equal(vc.frame, rp.frame)        # reading the frame composes it
    vc.close()
    assert np.array_equal(vc.frames, rp.close()) and not vc.is_color


# ------------------------------------------------------------------------------------------------ dirty memory
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


_REFS = {}


def test_ops_on_dirty_memory(hostile):
    from video import ops
    rng = _rng("dirty")
    frames = _frames(rng, 3, H, W, 1)
    layers = _layer_lists(rng, 3, H, W, 3, "mixed6")
    commands = list(_draw_cases(3).values())[:3]
    if "want" not in _REFS:                          # computed once for both fill bytes
        composed = K.compose_layers(frames, layers, color=True)
        _REFS["want"] = (composed, K.draw(composed, commands))
    for run in (1, 2):
        got = ops.compose_layers(frames, layers, color=True)
        assert np.array_equal(got, _REFS["want"][0]), run
        assert np.array_equal(ops.draw(got, commands), _REFS["want"][1]), run
        dev = ops.compose_layers(frames, layers, color=True, keep=True)       # the resident path
        assert np.array_equal(ops.draw(dev, commands), _REFS["want"][1]), run
