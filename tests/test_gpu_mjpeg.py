"""GPU: the batched JPEG encoder (va_jpeg_encode_u8, ops.jpeg_encode) and the Motion-JPEG writer behind the composer,
byte for byte against the NumPy restatement tests/jpeg_checks.py ("Motion-JPEG").  The fixture
tests/golden/mjpeg_v1.npz holds the small frames and the restatement's bytes for them (Pillow decoded those bytes
when the fixture was written); the large cases are restated here, once.  No tolerances."""
import os

import numpy as np
import pytest

import jpeg_checks as J

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu():
    from video import _hip
    return _hip.lib()


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "mjpeg_v1.npz"), allow_pickle=False)


def _same(got, want):
    """np.array_equal on the bytes"""
    return np.array_equal(np.frombuffer(bytes(got), np.uint8), np.frombuffer(bytes(want), np.uint8))


def _fixture_groups(fixture):
    """the fixture's cases grouped into stacks of one shape and quality: {(shape, quality): [names]}"""
    groups = {}
    for name in fixture["names"]:
        key = (fixture["frame_" + name].shape, int(fixture["quality_" + name]))
        groups.setdefault(key, []).append(str(name))
    return groups


def _check_fixture(fixture):
    from video import ops
    seen = 0
    for (shape, quality), names in _fixture_groups(fixture).items():
        stack = np.stack([fixture["frame_" + n] for n in names])
        got = ops.jpeg_encode(stack, quality, color=len(shape) == 3)
        assert len(got) == len(names)
        for n, g in zip(names, got):
            assert _same(g, fixture["bytes_" + n].tobytes()), (n, quality)
            seen += 1
        # frame k of a batch is frame k encoded alone
        alone = ops.jpeg_encode(stack[-1], quality, color=len(shape) == 3)
        assert len(alone) == 1 and _same(alone[0], got[-1]), (shape, quality)
    assert seen == len(fixture["names"]) == 120


def test_fixture_cases_equal_the_restatement(gpu, fixture):
    """1 x 1, 8 x 8, 9 x 17, 7 x 64, 80 x 16 and 37 x 53 in monochrome and colour: noise at qualities 1, 50, 90 and
    100, all 0, all 255, a flat frame, the two checkerboards and the blocks whose only AC coefficient is the last"""
    stuffed = sum(fixture["bytes_" + n].tobytes().count(b"\xff\x00") for n in fixture["names"] if n.startswith("noise"))
    assert stuffed > 100                              # the noise streams hold stuffed 0xFF bytes
    _check_fixture(fixture)


@pytest.fixture(scope="module")
def wide():
    """8 x 16384 noise at quality 100: a segment of some 200 (monochrome) and 540 (colour) KB, many LDS chunks"""
    rng = np.random.default_rng(16384)
    frames = {1: rng.integers(0, 256, (8, 16384), dtype=np.uint8), 3: rng.integers(0, 256, (8, 16384, 3), dtype=np.uint8)}
    return {c: (f, J.encode_frame(f, 100)) for c, f in frames.items()}


@pytest.mark.parametrize("c", (1, 3))
def test_a_segment_larger_than_any_lds_chunk(gpu, wide, c):
    from video import ops
    frame, want = wide[c]
    assert len(want) > 65536 * 3
    got = ops.jpeg_encode(frame, 100, color=c == 3)
    assert _same(got[0], want)


def test_more_frames_than_a_grid_dimension(gpu, fixture):
    """70 000 frames of 8 x 8, cycling through the fixture's 8 x 8 monochrome cases of quality 90"""
    from video import ops
    names = [n for n in fixture["names"] if n.endswith("_8x8x1") and int(fixture["quality_" + n]) == 90]
    assert len(names) >= 4
    n = 70000
    pick = np.arange(n) % len(names)
    stack = np.stack([fixture["frame_" + m] for m in names])[pick]
    blob, offsets = ops.jpeg_encode(stack, 90, ret_packed=True)
    parts = [fixture["bytes_" + m] for m in names]
    assert np.array_equal(np.diff(offsets), np.array([len(p) for p in parts])[pick])
    assert np.array_equal(blob, np.concatenate([parts[k] for k in pick]))


def _abi_run(L, stack, quality, cap, fill=0xA5):
    """va_jpeg_encode_u8 on raw buffers filled with `fill`: dict of the downloaded outputs"""
    from video import _hip, ops
    n, h, w = stack.shape[:3]
    c = 3 if stack.ndim == 4 else 1
    tables = ops.jpeg_tables(quality)
    head = np.frombuffer(ops.jpeg_header(h, w, c, quality), np.uint8)
    ins = dict(frames=stack, qt=np.concatenate(tables), head=head)
    dev = {k: _hip.DeviceBuffer.from_array(v) for k, v in ins.items()}
    outs = dict(sizes=(n, np.int64), offsets=(n + 1, np.int64), total=(1, np.int64), out=(max(cap, 1), np.uint8))
    for k, (m, dt) in outs.items():
        dev[k] = _hip.DeviceBuffer(m * np.dtype(dt).itemsize)
        _hip.check(L.va_memset(dev[k].ptr, fill, dev[k].nbytes, None))
    _hip.check(L.va_jpeg_encode_u8(dev["frames"].ptr, n, h, w, c, dev["qt"].ptr, dev["head"].ptr, len(head),
                                   dev["sizes"].ptr, dev["offsets"].ptr, dev["total"].ptr, dev["out"].ptr, cap, None))
    res = {k: dev[k].download((m,), dt) for k, (m, dt) in outs.items()}
    for b in dev.values():
        b.free()
    return res


@pytest.mark.parametrize("c", (1, 3))
def test_overflow_is_reported_and_nothing_written(gpu, fixture, c):
    names = [n for n in fixture["names"] if n.endswith("_37x53x%d" % c) and int(fixture["quality_" + n]) == 90]
    stack = np.stack([fixture["frame_" + n] for n in names])
    want = [fixture["bytes_" + n] for n in names]
    total = sum(len(w) for w in want)
    offsets = np.concatenate([[0], np.cumsum([len(w) for w in want])])
    short = _abi_run(gpu, stack, 90, total - 1)
    assert short["total"][0] == total and np.array_equal(short["offsets"], offsets)
    assert np.array_equal(short["sizes"], np.diff(offsets))
    assert np.all(short["out"] == 0xA5)                                       # too small by one byte: none written
    full = _abi_run(gpu, stack, 90, total)
    assert full["total"][0] == total and np.array_equal(full["out"], np.concatenate(want))
    assert np.array_equal(full["offsets"], offsets) and np.array_equal(full["sizes"], np.diff(offsets))
    again = _abi_run(gpu, stack, 90, total, fill=0x00)                         # two runs: identical bytes
    for key in full:
        assert full[key].tobytes() == again[key].tobytes(), key
    roomy = _abi_run(gpu, stack, 90, total + 64)
    assert np.array_equal(roomy["out"][:total], full["out"]) and np.all(roomy["out"][total:] == 0xA5)


def test_retry_through_ops(gpu, fixture, monkeypatch):
    from video import _hip, ops

    class Counting(object):
        """the library with its va_jpeg_encode_u8 calls counted: (capacity asked for) of each"""
        caps = []

        def __getattr__(self, name):
            fn = getattr(gpu, name)
            if name != "va_jpeg_encode_u8":
                return fn

            def counted(*args):
                self.caps.append(args[12])
                return fn(*args)
            return counted
    proxy = Counting()
    monkeypatch.setattr(_hip, "lib", lambda device=None: proxy)
    flat, flat_want = fixture["frame_flat_37x53x3"], fixture["bytes_flat_37x53x3"].tobytes()
    assert all(_same(g, flat_want) for g in ops.jpeg_encode(np.stack([flat] * 3), 90))
    assert len(proxy.caps) == 1 and proxy.caps[0] >= 3 * len(flat_want)        # the estimate had room: one launch
    del proxy.caps[:]
    frame, want = fixture["frame_noise_q100_37x53x3"], fixture["bytes_noise_q100_37x53x3"].tobytes()
    total = 3 * len(want)
    got = ops.jpeg_encode(np.stack([frame] * 3), 100)                          # noise at quality 100 needs more
    assert len(proxy.caps) == 2 and proxy.caps[0] < total and proxy.caps[1] == total      # once more, with exact room
    assert len(got) == 3 and all(_same(g, want) for g in got)


def test_device_frames_in(gpu, fixture, monkeypatch):
    from video import ops
    names = [n for n in fixture["names"] if n.endswith("_9x17x3") and int(fixture["quality_" + n]) == 90]
    stack = np.stack([fixture["frame_" + n] for n in names])
    dev = ops.DeviceFrames.upload(stack)
    uploads = []
    real = ops._Lease.upload
    monkeypatch.setattr(ops._Lease, "upload", lambda self, arr: uploads.append(arr.nbytes) or real(self, arr))
    try:
        got = ops.jpeg_encode(dev, 90)
        assert dev.buf is not None and np.array_equal(dev.download(), stack)   # it stays the caller's, untouched
    finally:
        dev.release()
    assert uploads == [128 + len(ops.jpeg_header(9, 17, 3, 90))]               # the tables and the header only
    for n, g in zip(names, got):
        assert _same(g, fixture["bytes_" + n].tobytes()), n
    with pytest.raises(ValueError):
        ops.jpeg_encode(stack, 90, color=False)
    with pytest.raises(TypeError):
        ops.jpeg_encode(stack.astype(np.int16), 90)
    assert ops.jpeg_encode(np.zeros((0, 8, 8), np.uint8)) == []


@pytest.mark.parametrize("fill", (0xFF, 0xA5), ids=["fill_ff", "fill_a5"])
def test_on_filled_memory_with_guarded_tails(gpu, fixture, wide, fill):
    """every case again with the test fill mode on: undefined device memory holds the fill byte and every buffer
    has a guarded tail ("Hostile memory")"""
    from video import _hip, ops
    ops.pool_clear()
    _hip.set_fill_mode(fill)
    try:
        for _ in (1, 2):                                                       # the second round gets recycled buffers
            _check_fixture(fixture)
        for c in (1, 3):
            assert _same(ops.jpeg_encode(wide[c][0], 100, color=c == 3)[0], wide[c][1])
        frame, want = fixture["frame_noise_q100_37x53x3"], fixture["bytes_noise_q100_37x53x3"].tobytes()
        assert all(_same(g, want) for g in ops.jpeg_encode(np.stack([frame] * 3), 100))     # the retry
        found = _hip.check_guards()
    finally:
        _hip.set_fill_mode(-1)
        ops.pool_clear()
        _hip.check_guards()
    assert found == [], found


@pytest.mark.parametrize("is_color", (False, True))
def test_composer_writes_a_clip_to_an_avi_file(gpu, tmp_path, monkeypatch, is_color):
    """5 frames through VideoComposer with a file name: the file's frames are ops.jpeg_encode of the composed frames"""
    from video import ops
    from video.io.backend_mjpeg import VideoMJPEG
    from video.io.composer import VideoComposer
    rng = np.random.default_rng(5)
    h, w = 45, 70
    shape = (h, w, 3) if is_color else (h, w)
    frames = rng.integers(0, 200, (5,) + shape, dtype=np.uint8)
    masks = rng.random((5, h, w)) < 0.3

    def compose(sink, **kwargs):
        vc = VideoComposer(sink, (w, h), 25, is_color, **kwargs)
        for f, m in zip(frames, masks):
            vc.set_frame(f)
            vc.highlight_mask(m, strength=90)
            vc.add_circle((30, 20), 9, "r", thickness=1)
            vc.add_rectangle((5, 6, 40, 30), "w")
        vc.close()
        return vc
    composed = compose(None).frames
    path = str(tmp_path / "clip.avi")
    calls, downloads = [], []
    real, real_download = ops.jpeg_encode, ops.DeviceFrames.download
    with monkeypatch.context() as patch:
        patch.setattr(ops, "jpeg_encode", lambda frames, **kw: calls.append(type(frames).__name__) or real(frames, **kw))
        patch.setattr(ops.DeviceFrames, "download",
                      lambda self, stream=None: downloads.append(self.shape) or real_download(self, stream))
        vc = compose(path, quality=80)
    assert vc.frames_written == 5 and calls == ["DeviceFrames"] and downloads == []     # only compressed bytes came back
    want = ops.jpeg_encode(composed, 80, color=is_color)
    assert all(_same(w_, J.encode_frame(f, 80)) for w_, f in zip(want, composed))
    with VideoMJPEG(path) as video:
        assert video.frame_count == 5 and video.size == (w, h) and video.fps == 25 and video.is_color == is_color
        for k in range(5):
            assert _same(video.get_frame_bytes(k), want[k]), k
    J.parse_avi(open(path, "rb").read())
