"""CPU: the host layer of annotating on the device ("Annotating on the device").

`VideoComposer.annotate_frames` with `ops.DeviceFrames`, `ops.DeviceContours`, `ops.find_contours`,
`ops.compose_layers`, `ops.draw_contours` and `ops.draw` replaced through monkeypatch by host stand-ins over the
restatement tests/composer_checks.py and the oracle's contour scanner (the composer looks them up on video.ops when
it runs); the table and map checks of `ops._compose_tables` and `ops.draw_contours`, which need no device; and the
binding of `va_draw_contours_u8` against the header's argument list."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import composer_checks as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 12, 17


# ------------------------------------------------------------------------------------------------ stand-ins
class FakeFrames(object):
    """ops.DeviceFrames on the host: the stack is an array"""
    log = None

    def __init__(self, arr):
        self.arr = np.array(arr, np.uint8, copy=True)
        self.released = False

    n = property(lambda self: self.arr.shape[0])
    h = property(lambda self: self.arr.shape[1])
    w = property(lambda self: self.arr.shape[2])
    c = property(lambda self: 3 if self.arr.ndim == 4 else 1)
    shape = property(lambda self: tuple(self.arr.shape))
    nbytes = property(lambda self: self.arr.nbytes)

    @classmethod
    def upload(cls, frames, stream=None):
        cls.log.append(("upload", len(frames)))
        return cls(frames)

    def gather(self, indices, stream=None):
        self.log.append(("gather", list(indices)))
        return FakeFrames(self.arr[list(indices)])

    def download(self, stream=None):
        assert not self.released
        return self.arr.copy()

    def release(self):
        self.released = True


class FakeContours(object):
    """ops.DeviceContours on the host: the per-frame lists of the oracle's scanner"""

    def __init__(self, masks):
        from oracle import oracle as O
        self.lists = [O.find_contours_external_simple(m) for m in masks]
        self.n, (self.h, self.w) = len(masks), masks.shape[1:]
        self.released = False

    def release(self):
        self.released = True


@pytest.fixture
def fakes(monkeypatch):
    """video.ops with host stand-ins; the calls are logged"""
    from video import ops
    log = []
    FakeFrames.log = log

    def plane(operand):
        if isinstance(operand, tuple) and isinstance(operand[0], FakeFrames):
            return operand[0].arr[operand[1]]
        return operand

    def arrays(frames):
        return frames.arr if isinstance(frames, FakeFrames) else np.asarray(frames)

    def compose_layers(frames, layers, color=None, keep=False, stream=None):
        assert keep
        log.append(("layers", len(arrays(frames)), sum(len(x) for x in layers)))
        plain = [[(l[0], plane(l[1])) + tuple(l[2:]) for l in frame] for frame in layers]
        return FakeFrames(K.compose_layers(arrays(frames), plain, color=color))

    def draw(frames, commands, keep=False, stream=None):
        assert keep
        log.append(("draw", len(arrays(frames)), sum(len(x) for x in commands)))
        return FakeFrames(K.draw(arrays(frames), commands))

    def find_contours(masks, ret_info=False, moments=False, stream=None, keep=False):
        assert isinstance(masks, FakeFrames) and keep
        log.append(("find", masks.n))
        return FakeContours(masks.arr)

    def draw_contours(frames, contours, color, frame_map=None, keep=False, stream=None):
        assert isinstance(frames, FakeFrames) and isinstance(contours, FakeContours) and keep
        log.append(("contours", frames.n, None if frame_map is None else np.asarray(frame_map).tolist()))
        targets = range(contours.n) if frame_map is None else frame_map
        commands = [[] for _ in range(frames.n)]
        for f, t in enumerate(targets):
            if t >= 0:
                commands[t] += [("polyline", c, True, color) for c in contours.lists[f]]
        frames.arr = K.draw(frames.arr, commands)
        return frames

    def refuse(*args, **kwargs):
        raise AssertionError("this test must not reach the device")
    monkeypatch.setattr(ops, "DeviceFrames", FakeFrames)
    monkeypatch.setattr(ops, "DeviceContours", FakeContours)
    monkeypatch.setattr(ops, "compose_layers", compose_layers)
    monkeypatch.setattr(ops, "draw", draw)
    monkeypatch.setattr(ops, "find_contours", find_contours)
    monkeypatch.setattr(ops, "draw_contours", draw_contours)
    monkeypatch.setattr(ops, "resize", refuse)
    return log


def _clip(n, color=False, seed=5):
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (n, H, W) + ((3,) if color else ()), dtype=np.uint8)
    yy, xx = np.mgrid[:H, :W]
    masks = np.stack([((xx - 4 - t % 5) ** 2 + (yy - 5) ** 2 < 9) | ((abs(xx - 12) < 3) & (abs(yy - 8 + t % 3) < 2))
                      for t in range(n)])
    return frames, masks


def _loop(target, frames, masks, channel, strength, contours, color, lists=None):
    """the loop of the issue, on a VideoComposer or on the restatement's Replay"""
    for i in range(len(frames)):
        target.set_frame(frames[i])
        if masks is not None:
            target.highlight_mask(masks[i], channel, strength)
        if contours:
            target.add_contour(lists[i], color)


def _replay(is_color, period=1):
    from video.io.composer import get_color
    return K.Replay((W, H), is_color, output_period=period, get_color=get_color)


def _lists(masks):
    from oracle import oracle as O
    return [O.find_contours_external_simple(m) for m in masks]


# ------------------------------------------------------------------------------------------------ rounds
@pytest.mark.parametrize("is_color", (False, True))
def test_rounds_of_one_batch(fakes, is_color):
    from video.io.composer import VideoComposer
    frames, masks = _clip(5)
    vc = VideoComposer(None, (W, H), 25, is_color)
    vc.annotate_frames(frames, masks, "all", 100, contours=True, color="r")
    # the frames and the masks go up once each, one find, one layer pass with a layer per frame, one contour pass
    assert fakes == [("upload", 5), ("upload", 5), ("find", 5), ("layers", 5, 5), ("contours", 5, None)]
    rp = _replay(is_color)
    _loop(rp, frames, masks, "all", 100, True, "r", _lists(masks))
    assert np.array_equal(vc.frames, rp.close()) and vc.frames_written == 5 and vc.next_frame == 4
    assert vc.frame is None                         # no current frame after a batch
    with pytest.raises(RuntimeError):
        vc.add_circle((2, 2), 1)
    del fakes[:]
    vc.annotate_frames(FakeFrames(frames), None)    # no masks, no contours: the layer pass alone (it converts to colour)
    assert fakes == [("gather", [0, 1, 2, 3, 4]), ("layers", 5, 0)] and vc.frames_written == 10
    want = np.repeat(frames[..., None], 3, axis=-1) if is_color else frames
    assert np.array_equal(vc.frames[5:], want)


def test_device_operands_stay_the_caller_s(fakes):
    from video.io.composer import VideoComposer
    frames, masks = _clip(4, color=True)
    dev, mdev = FakeFrames(frames), FakeFrames(masks.astype(np.uint8) * 200)
    found = FakeContours(masks)
    got = []

    class Sink(object):
        def write_frames(self, stack):
            assert isinstance(stack, FakeFrames) and not stack.released
            got.append(stack.download())
    vc = VideoComposer(Sink(), (W, H), 25, True)
    vc.annotate_frames(dev, mdev, "g", 30, contours=found, color="b")
    assert fakes == [("gather", [0, 1, 2, 3]), ("layers", 4, 4), ("contours", 4, None)]
    assert not (dev.released or mdev.released or found.released)
    assert np.array_equal(dev.arr, frames) and np.array_equal(mdev.arr, masks.astype(np.uint8) * 200)
    rp = _replay(True)
    _loop(rp, frames, masks, "g", 30, True, "b", found.lists)
    assert len(got) == 1 and np.array_equal(got[0], rp.close()) and vc.frames_written == 4


def test_pending_frames_are_flushed_first_and_calls_mix(fakes):
    from video.io.composer import VideoComposer
    frames, masks = _clip(9)
    lists = _lists(masks)
    sunk = []
    vc = VideoComposer(sunk.append, (W, H), 25, False, batch=4)
    rp = _replay(False)
    for target in (vc, rp):
        for i in (0, 1):
            target.set_frame(frames[i])
            target.add_circle((3 + i, 4), 2, "w")
    assert sunk == []
    vc.annotate_frames(frames[2:6], masks[2:6], contours=True, color="w")
    _loop(rp, frames[2:6], masks[2:6], "all", 128, True, "w", lists[2:6])
    assert len(sunk) == 6                           # the two pending frames first, then the batch
    assert [x[0] for x in fakes] == ["layers", "draw", "upload", "upload", "find", "layers", "contours"]
    for target in (vc, rp):
        target.set_frame(frames[6])
        target.highlight_mask(masks[6], "all", 10)
        target.add_rectangle((1, 1, 6, 5), "w")
    vc.annotate_frames(frames[7:9], None, contours=None)
    _loop(rp, frames[7:9], None, "all", 128, False, "w")
    vc.close()
    assert np.array_equal(np.array(sunk), rp.close()) and vc.frames_written == 9 and vc.next_frame == 8


@pytest.mark.parametrize("period", (1, 2, 3))
@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
def test_output_period_gathers_and_maps(fakes, period, device):
    """batches of 5, 4 and 6 frames: they start at next_frame + 1 = 0, 5 and 9, which are no multiples of 2 or 3"""
    from video.io.composer import VideoComposer
    frames, masks = _clip(15)
    lists = _lists(masks)
    vc = VideoComposer(None, (W, H), 25, False, output_period=period)
    rp = _replay(False, period)
    for start, stop in ((0, 5), (5, 9), (9, 15)):
        del fakes[:]
        n = stop - start
        chosen = [i for i in range(n) if (start + i) % period == 0]
        f, m = frames[start:stop], masks[start:stop]
        given = FakeContours(m) if device else True
        vc.annotate_frames(FakeFrames(f) if device else f, FakeFrames(m.astype(np.uint8)) if device else m, "all", 77,
                           contours=given, color="w")
        _loop(rp, f, m, "all", 77, True, "w", lists[start:stop])
        assert vc.next_frame == stop - 1
        fmap = np.full(n, -1)
        fmap[chosen] = np.arange(len(chosen))
        if device:                                  # gathered on the device; the contours of all n frames are mapped
            assert fakes[0] == ("gather", chosen) and fakes[1] == ("layers", len(chosen), len(chosen))
            assert fakes[2] == ("contours", len(chosen), None if len(chosen) == n else fmap.tolist())
        else:                                       # only the chosen frames and masks go up: the identity
            assert fakes[:3] == [("upload", len(chosen)), ("upload", len(chosen)), ("find", len(chosen))]
            assert fakes[4] == ("contours", len(chosen), None)
    assert np.array_equal(vc.frames, rp.close()) and len(vc.frames) == len(range(0, 15, period))


def test_a_batch_without_output_frames_does_nothing(fakes):
    from video.io.composer import VideoComposer
    frames, _ = _clip(3)
    vc = VideoComposer(None, (W, H), 25, False, output_period=5)
    vc.annotate_frames(frames[:1])
    vc.annotate_frames(frames, "no masks at all", "nonsense", 999)      # frames 1 .. 3: skipped before any check
    assert vc.next_frame == 3 and vc.frames_written == 1 and fakes == [("upload", 1), ("layers", 1, 0)]


# ------------------------------------------------------------------------------------------------ errors
def test_errors(fakes):
    from video.io.composer import VideoComposer
    frames, masks = _clip(3)
    rgb = np.repeat(frames[..., None], 3, axis=-1)
    mono, color = VideoComposer(None, (W, H), 25, False), VideoComposer(None, (W, H), 25, True)
    for call in (lambda: mono.annotate_frames(rgb),                                     # colour into monochrome
                 lambda: mono.annotate_frames(FakeFrames(rgb)),
                 lambda: mono.annotate_frames(frames[:, :5]), lambda: mono.annotate_frames(frames[0]),
                 lambda: color.annotate_frames(np.zeros((3, H, W, 2), np.uint8)),
                 lambda: mono.annotate_frames(frames, masks[:2]), lambda: mono.annotate_frames(frames, masks[:, :4]),
                 lambda: mono.annotate_frames(frames, FakeFrames(rgb)),
                 lambda: mono.annotate_frames(frames, masks, "r"),                      # a channel on monochrome
                 lambda: color.annotate_frames(frames, masks, "x"),
                 lambda: color.annotate_frames(frames, masks, "all", 256),
                 lambda: color.annotate_frames(frames, masks, "all", 12.5),
                 lambda: mono.annotate_frames(frames, None, contours=True),             # no masks to find them in
                 lambda: mono.annotate_frames(frames, masks, contours=FakeContours(masks[:2])),
                 lambda: mono.annotate_frames(frames, masks, contours=FakeContours(masks[:, :5])),
                 lambda: mono.annotate_frames(frames, masks, contours=True, color="no such colour")):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: mono.annotate_frames(frames.astype(np.float32)),
                 lambda: mono.annotate_frames(frames, masks, contours=_lists(masks))):
        with pytest.raises(TypeError):
            call()
    zoomed = VideoComposer(None, (W, H), 25, False, zoom_factor=2)
    with pytest.raises(NotImplementedError, match="zoom_factor"):
        zoomed.annotate_frames(frames)
    assert fakes == [] and mono.next_frame == -1 and color.next_frame == -1      # nothing ran, nothing advanced
    assert color.get_color("g") == [0, 127, 0] and mono.get_color("g") == 42     # colour into monochrome: the mean


# ------------------------------------------------------------------------------------------------ the tables
def _stack(n, c=1, h=H, w=W):
    from video import ops
    return ops.DeviceFrames(None, n, h, w, c)       # the tables never touch the buffer


def test_compose_tables_with_device_planes():
    from video import ops
    masks, images, rgb = _stack(4), _stack(3), _stack(2, 3)
    layers = [[("highlight", (masks, 2), None, 50)], [("blend", (images, 1), 0.5, (masks, 0)), ("add", (images, 2), None)],
              [("highlight", (masks, 3), "g", 9)]]
    table, off, im, mk = ops._compose_tables(layers, 3, H, W, 3, "test")
    assert im is images and mk is masks and off.tolist() == [0, 1, 3, 4]
    assert table["mask_off"].tolist() == [2 * H * W, 0, -1, 3 * H * W]
    assert table["image_off"].tolist() == [0, H * W, 2 * H * W, 0] and table["image_channels"].tolist() == [0, 1, 1, 0]
    table, _, im, mk = ops._compose_tables([[("add", (rgb, 1), None)]], 1, H, W, 3, "test")
    assert im is rgb and mk is None and table["image_off"].tolist() == [3 * H * W] and table["image_channels"][0] == 3
    host_mask, host_image = np.ones((H, W), bool), np.zeros((H, W), np.uint8)
    # device and host planes of different roles mix; of the same role they do not
    table, _, im, mk = ops._compose_tables([[("add", host_image, (masks, 1))]], 1, H, W, 1, "test")
    assert mk is masks and isinstance(im, np.ndarray) and table["mask_off"][0] == H * W
    for bad in ([[("highlight", (masks, 0), None, 5), ("highlight", host_mask, None, 5)]],
                [[("add", (images, 0), None)], [("add", host_image, None)]],
                [[("highlight", (masks, 0), None, 5), ("highlight", (_stack(4), 0), None, 5)]],    # two stacks
                [[("add", (images, 0), None), ("blend", (_stack(3), 0), 0.5, None)]],
                [[("highlight", (masks, 4), None, 5)]], [[("highlight", (masks, -1), None, 5)]],    # the index
                [[("highlight", (masks, 1.5), None, 5)]],
                [[("highlight", (rgb, 0), None, 5)]],                                               # a colour mask
                [[("highlight", (_stack(4, 1, H, W + 1), 0), None, 5)]], [[("add", (_stack(3, 1, H + 1), 0), None)]]):
        with pytest.raises(ValueError):
            ops._compose_tables(bad + [[]] * (2 - len(bad)), 2, H, W, 3, "test")
    with pytest.raises(ValueError, match="color image"):
        ops._compose_tables([[("add", (rgb, 0), None)]], 1, H, W, 1, "test")


def test_draw_contours_checks_its_map_before_the_launch():
    from video import ops
    found = ops.DeviceContours(None, None, None, 4, H, W, np.zeros(4, np.int32), 0, 0)
    frames = np.zeros((3, H, W), np.uint8)
    assert ops._frame_map([2, -1, 0, 1], 4, 3, "t").dtype == np.int32
    assert ops._frame_map(None, 3, 3, "t") is None
    for fmap in ([0, 1, 2], [0, 1, 2, 0, 1], [0, 1, 2, 3], [0, -2, 1, 2], [[0, 1, 2, 0]], [0.0, 1.0, 2.0, 0.0], None):
        with pytest.raises(ValueError):
            ops.draw_contours(frames, found, 255, frame_map=fmap)
    with pytest.raises(ValueError):
        ops.draw_contours(frames, found, 256, frame_map=[0, 1, 2, -1])               # the colour
    with pytest.raises(ValueError):
        ops.draw_contours(np.zeros((3, H, W + 1), np.uint8), found, 1, frame_map=[0, 1, 2, -1])
    with pytest.raises(TypeError):
        ops.draw_contours(frames, [[]] * 3, 1)
    got = ops.draw_contours(frames, found, 1, frame_map=[0, 1, 2, -1])                # no contours: nothing to launch
    assert np.array_equal(got, frames) and got is not frames


def test_engine_refuses_other_names_in_keep():
    from video.engine import FrameEngine
    eng = FrameEngine.__new__(FrameEngine)          # the check needs no pipeline
    eng.dtype, eng.channels = np.dtype(np.uint8), 1
    assert eng._check_keep(("mask", "filtered")) == {"mask", "filtered"} and eng._check_keep(()) == set()
    for keep in (("labels",), ("mask", "counts"), "stats"):
        with pytest.raises(ValueError):
            eng._check_keep(keep)
    eng.dtype = np.dtype(np.float32)
    with pytest.raises(ValueError):
        eng._check_keep(("filtered",))
    eng._handle, eng._dev = None, {}


# ------------------------------------------------------------------------------------------------ the C ABI
def test_binding_matches_the_header():
    from video import _hip
    text = open(os.path.join(ROOT, "include", "videoanalysis_hip.h")).read()
    assert "video/io/composer.py:228-237" in text
    decl = re.search(r"int va_draw_contours_u8\((.*?)\);", text, re.S).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == [
        "frames_dev", "n_out", "h", "w", "c", "info_dev", "point_off_dev", "ncontours", "points_dev", "npoints",
        "frame_map_dev", "n_src", "color", "status_dev", "stream"]

    def ctype(p):
        if "*" in p:
            return C.c_void_p
        return {"int": C.c_int, "int64_t": C.c_int64, "uint32_t": C.c_uint32}[p.split()[0]]
    res, args = _hip.SIGNATURES["va_draw_contours_u8"]
    assert res is C.c_int and args == [ctype(p) for p in params]
    src = open(os.path.join(ROOT, "video-analysis_amd", "csrc", "va_compose.hip")).read()
    assert "int va_draw_contours_u8(" in src
