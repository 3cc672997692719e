"""GPU: 4:2:0 and 4:2:2 files through the batched JPEG decoder (va_jpeg_decode_sampled_u8, ops.jpeg_decode),
VideoMJPEG's device decoder and FrameEngine.run_frames, byte for byte against the NumPy restatement
tests/jpeg_subsampled_checks.py ("Subsampled Motion-JPEG decoding").  The fixture
tests/golden/mjpeg_subsampled_v1.npz holds the restatement's pixels and status words of the small streams; the large
cases are restated here, once.  No tolerances."""
import os
import struct

import numpy as np
import pytest

import jpeg_decode_checks as D
import jpeg_subsampled_checks as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu():
    from video import _hip
    return _hip.lib()


@pytest.fixture(scope="module")
def cases():
    """{'a' | 'b': [(name, bytes, expected pixels, expected status)]} of the fixture"""
    out, _ = S.fixture_cases(os.path.join(ROOT, "tests", "golden", "mjpeg_subsampled_v1.npz"))
    assert (len(out["a"]), len(out["b"])) == (200, 30)
    return out


def _by_header(items):
    """the cases grouped into batches of one header: [[case]]"""
    groups = {}
    for item in items:
        groups.setdefault(D.header_key(D.parse_header(item[1], sampling="any")), []).append(item)
    return list(groups.values())


def _check_valid(cases):
    from video import ops
    seen = shared = 0
    for batch in _by_header(cases["a"]):
        got, status = ops.jpeg_decode([data for _, data, _, _ in batch], ret_status=True)
        assert got.dtype == np.uint8 and len(got) == len(batch) and not status.any(), batch[0][0]
        for (name, _, want, _), g in zip(batch, got):
            assert np.array_equal(g, want), name
            seen += 1
        shared += len(batch) > 1
        alone = ops.jpeg_decode([batch[-1][1]])                      # frame k of a batch is frame k decoded alone
        assert alone.shape == (1,) + batch[-1][2].shape and np.array_equal(alone[0], batch[-1][2]), batch[-1][0]
    assert seen == 200 and shared >= 6                               # noise and smooth of one quality share a header
    # all streams of a shape in one call: ops.jpeg_decode cuts it into its runs of one header
    big = [c for c in cases["a"] if c[2].shape == (37, 53, 3)]
    got = ops.jpeg_decode([c[1] for c in big], color=True)
    assert all(np.array_equal(g, c[2]) for g, c in zip(got, big))


def test_valid_fixture_streams_equal_the_restatement(gpu, cases):
    """Pillow's 4:2:0 and 4:2:2 files of 1x1 .. 37x53: no restart markers, one per MCU row, one every 3 MCUs,
    optimised Huffman tables; two chroma columns (replication), three (the smallest triangle), exactly one MCU, one
    row and column beyond an MCU"""
    _check_valid(cases)


def _check_hostile(cases):
    from video import ops
    for name, data, want, want_status in cases["b"]:
        got, status = ops.jpeg_decode([data], ret_status=True)
        assert status.dtype == np.int32 and status[0] == want_status, (name, status, want_status)
        assert np.array_equal(got[0], want), name
        if want_status:
            with pytest.raises(ValueError) as err:
                ops.jpeg_decode([data])
            assert "frame 0" in str(err.value) and ops.jpeg_status_text(want_status) in str(err.value)
    # hostile frames between two good ones of their header change neither of them
    for layout in ("420", "422"):
        good = [c for c in cases["a"] if c[0] == layout + "_q50_37x53_rows"][0]
        batch = [good] + [c for c in cases["b"] if c[0].startswith(layout)] + [good]
        assert len(_by_header(batch)) == 1
        got, status = ops.jpeg_decode([c[1] for c in batch], ret_status=True)
        assert status.tolist() == [c[3] for c in batch]
        assert all(np.array_equal(g, c[2]) for g, c in zip(got, batch))


def test_hostile_streams_equal_the_restatement(gpu, cases):
    assert {s for _, _, _, s in cases["b"]} >= {0, 1, 2, 8, 12}
    _check_hostile(cases)


@pytest.fixture(scope="module")
def mixed():
    """frames of one shape that alternate 4:2:0, 4:4:4 and 4:2:2, and the restatement's decode of each"""
    rng = np.random.default_rng(420)
    frames = rng.integers(0, 256, (3, 24, 40, 3), dtype=np.uint8)
    import jpeg_checks as J
    streams = [S.encode_frame(frames[0], 90, (2, 2)), J.encode_frame(frames[1], 90), S.encode_frame(frames[2], 90, (2, 1))]
    streams = streams + streams[::-1] + streams
    want = [S.decode(s) for s in streams]
    assert not any(st for _, st in want)
    return streams, np.stack([px for px, _ in want])


def _check_mixed(mixed):
    from video import ops
    streams, want = mixed
    heads = [ops.jpeg_parse_header(s, sampling="any") for s in streams]
    assert [hd["sampling"] for hd in heads[:3]] == [(2, 2), (1, 1), (2, 1)]
    assert len(ops.jpeg_decode_groups(heads)) == 7                   # 420 444 422 422 444 420 420 444 422
    assert np.array_equal(ops.jpeg_decode(streams), want)


def test_a_batch_that_alternates_the_layouts(gpu, mixed):
    _check_mixed(mixed)


def _abi_run(L, batch, workspace_bytes=None, fill=0xA5, extra=0, plain=False):
    """va_jpeg_decode_sampled_u8 (plain: va_jpeg_decode_u8) on raw buffers filled with `fill`: (pixels with `extra`
    bytes behind them, status)"""
    from video import _hip, ops
    heads = [ops.jpeg_parse_header(data, sampling="any") for data in batch]
    head = heads[0]
    n, h, w, c, ri = len(batch), head["h"], head["w"], head["c"], head["ri"]
    lh, lv = head["sampling"]
    tables = b"".join(ops._jpeg_decode_table(*dc) + ops._jpeg_decode_table(*ac) for dc, ac in head["huff"])
    offsets = np.concatenate([[0], np.cumsum([len(d) for d in batch])]).astype(np.int64)
    ins = dict(bytes=np.frombuffer(b"".join(batch), np.uint8), offsets=offsets,
               scan=np.array([hd["scan_begin"] for hd in heads], np.int64), qt=head["qtables"].ravel(),
               huff=np.frombuffer(tables, np.uint8))
    dev = {k: _hip.DeviceBuffer.from_array(v) for k, v in ins.items()}
    full = int(L.va_jpeg_decode_sampled_workspace_bytes(n, h, w, c, ri, lh, lv))
    room = full if workspace_bytes is None else workspace_bytes
    outs = dict(out=(n * h * w * c + extra, np.uint8), status=(n, np.int32), ws=(room, np.uint8))
    for k, (m, dt) in outs.items():
        dev[k] = _hip.DeviceBuffer(m * np.dtype(dt).itemsize)
        _hip.check(L.va_memset(dev[k].ptr, fill, dev[k].nbytes, None))
    try:
        front = (dev["bytes"].ptr, dev["offsets"].ptr, dev["scan"].ptr, n, h, w, c, ri)
        back = (dev["qt"].ptr, dev["huff"].ptr, len(tables), dev["out"].ptr, dev["status"].ptr, dev["ws"].ptr, room, None)
        if plain:
            _hip.check(L.va_jpeg_decode_u8(*(front + back)))
        else:
            _hip.check(L.va_jpeg_decode_sampled_u8(*(front + (lh, lv) + back)))
        return dev["out"].download((outs["out"][0],), np.uint8), dev["status"].download((n,), np.int32)
    finally:
        for b in dev.values():
            b.free()


def _check_forwarding(gpu):
    """1 x 1 through the new entry: the bytes and status words of va_jpeg_decode_u8, colour and monochrome, with a
    hostile frame in the batch"""
    enc = np.load(os.path.join(ROOT, "tests", "golden", "mjpeg_v1.npz"), allow_pickle=False)
    dec = np.load(os.path.join(ROOT, "tests", "golden", "mjpeg_decode_v1.npz"), allow_pickle=False)
    for source in ("noise_q90_37x53x3", "noise_q50_37x53x1"):
        batch = [enc["bytes_" + source].tobytes(), dec["c_bytes_%s_cut_mid" % source].tobytes(),
                 dec["c_bytes_%s_ff00" % source].tobytes()]
        old = _abi_run(gpu, batch, extra=64, plain=True)
        new = _abi_run(gpu, batch, extra=64)
        assert old[0].tobytes() == new[0].tobytes() and old[1].tobytes() == new[1].tobytes() and old[1][1:].all()
        assert np.array_equal(new[0][:37 * 53 * (3 if source.endswith("3") else 1)].reshape(D.decode(batch[0])[0].shape),
                              D.decode(batch[0])[0])


def test_the_new_entry_with_1x1_writes_what_the_plain_entry_writes(gpu):
    _check_forwarding(gpu)


@pytest.fixture(scope="module")
def encoded():
    """from the restated encoder at quality 100, with a restart interval per MCU row and with none: 32 x 64 (every
    pixel row complete and aligned) and 16 x 1040 (130 luma blocks a row: three waves; 520 chroma columns), both
    layouts; with the restatement's decode: [(name, bytes, pixels)]"""
    rng = np.random.default_rng(1040)
    out = []
    for h, w in ((32, 64), (16, 1040)):
        frame = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        for hv in S.LAYOUTS:
            first = None
            for ri in (None, 0):
                data = S.encode_frame(frame, 100, hv, ri)
                head = D.parse_header(data, sampling="any")
                assert head["nseg"] == (1 if ri == 0 else -(-h // (8 * hv[1])))
                pixels, status = S.decode(data, head)
                assert status == 0
                first = pixels if first is None else first
                assert np.array_equal(pixels, first)
                out.append(("%dx%d %s ri %s" % (h, w, hv, ri), data, pixels))
    return out


def _check_encoded(encoded):
    from video import ops
    for name, data, want in encoded:
        assert np.array_equal(ops.jpeg_decode([data, data], color=True), np.stack([want, want])), name


def test_aligned_rows_and_rows_of_three_waves(gpu, encoded):
    _check_encoded(encoded)


def _check_many_frames(cases):
    from video import ops
    name, data, want, _ = [c for c in cases["a"] if c[0] == "420_q1_16x16_plain"][0]
    n = 70000
    blob = np.tile(np.frombuffer(data, np.uint8), n)
    got = ops.jpeg_decode((blob, np.arange(n + 1, dtype=np.int64) * len(data)))
    assert got.shape == (n, 16, 16, 3) and (got == want[None]).all()


def test_more_frames_than_a_grid_dimension(gpu, cases):
    """70 000 copies of one 16 x 16 4:2:0 stream"""
    _check_many_frames(cases)


def _check_chunks(gpu, cases, layout, monkeypatch):
    from video import _hip, ops
    source = layout + "_q50_37x53_rows"
    good = [c for c in cases["a"] if c[0] == source][0]
    hostile = [c for c in cases["b"] if c[0].startswith(source)]
    batch = [good] + hostile[:3] + [good] + hostile[-3:]
    assert len(batch) == 8 and any(x[3] for x in batch) and len(_by_header(batch)) == 1
    data = [x[1] for x in batch]
    want = np.concatenate([x[2].ravel() for x in batch])
    pixels, status = _abi_run(gpu, data, extra=64)
    assert np.array_equal(pixels[:-64], want) and np.all(pixels[-64:] == 0xA5)
    assert status.tolist() == [x[3] for x in batch]
    a = (37, 53, 3, 4) + D.parse_header(good[1], sampling="any")["sampling"]
    size = lambda n: int(gpu.va_jpeg_decode_sampled_workspace_bytes(n, *a))
    three = size(3)
    assert three * 2 < size(8)
    chunked = _abi_run(gpu, data, workspace_bytes=three, fill=0x00, extra=64)
    assert np.array_equal(chunked[0][:-64], pixels[:-64]) and np.array_equal(chunked[1], status)
    assert not chunked[0][-64:].any()
    again = _abi_run(gpu, data, extra=64)
    assert again[0].tobytes() == pixels.tobytes() and again[1].tobytes() == status.tobytes()
    with pytest.raises(_hip.HipError) as err:                       # VA_ERR_RANGE: not even one frame fits
        _abi_run(gpu, data, workspace_bytes=size(1) - 256)
    assert err.value.code == -34 and "one frame" in str(err.value)
    # the same through ops.jpeg_decode's own (pooled) workspace, capped at what 3 frames need
    asked = []

    class Counting(object):
        def __getattr__(self, name):
            fn = getattr(gpu, name)
            if name not in ("va_jpeg_decode_u8", "va_jpeg_decode_sampled_u8"):
                return fn

            def counted(*args):
                asked.append((name, args[3], args[-2]))
                return fn(*args)
            return counted
    with monkeypatch.context() as patch:
        patch.setattr(ops, "JPEG_DECODE_WORKSPACE_MAX", three)
        patch.setattr(_hip, "lib", lambda device=None: Counting())
        got, got_status = ops.jpeg_decode(data, ret_status=True)
    assert asked == [("va_jpeg_decode_sampled_u8", 8, three)]
    assert np.array_equal(got.ravel(), want) and got_status.tolist() == [x[3] for x in batch]


@pytest.mark.parametrize("layout", ("420", "422"))
def test_chunks_two_runs_and_a_roomy_buffer(gpu, cases, layout, monkeypatch):
    """a workspace that holds 3 of 8 frames (three chunks) gives the bytes of the single-chunk run, at the ABI and
    through ops.jpeg_decode with its workspace cap lowered; VA_ERR_RANGE below one frame; two runs write identical
    bytes; the bytes behind the last frame stay as they were.  Hostile frames ride along."""
    _check_chunks(gpu, cases, layout, monkeypatch)


def _write_avi(path, streams, size, fps=25):
    """an AVI 1.0 file with one MJPG stream and an idx1 around stored JPEG files"""
    chunk = lambda cc, payload: cc + struct.pack("<I", len(payload)) + payload + b"\0" * (len(payload) & 1)
    movi, index = b"movi", []
    for s in streams:
        index.append(struct.pack("<4sIII", b"00dc", 0x10, len(movi), len(s)))
        movi += chunk(b"00dc", s)
    w, h = size
    avih = struct.pack("<14I", 1000000 // fps, 0, 0, 0x10, len(streams), 0, 1, max(len(s) for s in streams), w, h,
                       0, 0, 0, 0)
    strh = struct.pack("<4s4sIHHIIIIIIIIhhhh", b"vids", b"MJPG", 0, 0, 0, 0, 1, fps, 0, len(streams), 0, 0xFFFFFFFF, 0,
                       0, 0, w, h)
    strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0)
    hdrl = b"hdrl" + chunk(b"avih", avih) + chunk(b"LIST", b"strl" + chunk(b"strh", strh) + chunk(b"strf", strf))
    body = b"AVI " + chunk(b"LIST", hdrl) + chunk(b"LIST", movi) + chunk(b"idx1", b"".join(index))
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def _check_video_file(cases, tmp_path):
    from video import ops
    from video.engine import FrameEngine
    from video.io.backend_mjpeg import VideoMJPEG
    from video.io.file import load_any_video
    picks = [c for c in cases["a"] if c[0].startswith("420") and c[2].shape == (37, 53, 3)]
    assert len(picks) == 20
    picks = picks + picks[::-1]                                      # 40 frames; the headers change along the file
    path = str(tmp_path / "camera.avi")
    _write_avi(path, [c[1] for c in picks], (53, 37))
    want = np.stack([c[2] for c in picks])
    calls = []
    real = ops.jpeg_decode
    video = load_any_video(path, {"decoder": "device"})
    try:
        ops.jpeg_decode = lambda streams, **kw: calls.append(len(streams)) or real(streams, **kw)
        assert isinstance(video, VideoMJPEG) and video.frame_count == 40 and video.is_color and video.size == (53, 37)
        assert [video.get_frame_bytes(k) for k in (0, 39)] == [picks[0][1], picks[39][1]]
        got = np.stack([f for f in video])
        assert np.array_equal(got, want) and calls == [32, 8]
        del calls[:]
        for k in (39, 3, 33, -1, -40, 31, 32):
            assert np.array_equal(video[k], want[k]), k
        assert calls == [32, 8, 32, 8]
        del calls[:]
        assert np.array_equal(video.get_frames(10, 37), want[10:37]) and calls == [27]
        dev = video.get_device_frames(30, None)
        try:
            assert isinstance(dev, ops.DeviceFrames) and dev.shape == (10, 37, 53, 3)
            host = dev.download()
            assert np.array_equal(host, want[30:])
            kw = dict(size=(53, 37), channels=1, max_batch=16, sigma=1.0, thresh=100,
                      prepare={"src_size": (53, 37), "src_channels": 3, "mono": "mean"})
            expect = FrameEngine(**kw).run(host, want=("filtered", "mask"))
            result = FrameEngine(**kw).run_frames(dev, want=("filtered", "mask"))
            assert sorted(result) == sorted(expect) and 0 < expect["mask"].mean() < 255
            for key in expect:
                assert np.array_equal(result[key], expect[key]), key
            assert np.array_equal(dev.download(), host)                 # the stack stays the caller's, untouched
        finally:
            dev.release()
    finally:
        ops.jpeg_decode = real
        video.close()


def test_a_camera_style_file_with_the_device_decoder(gpu, cases, tmp_path):
    """a 40-frame AVI of 4:2:0 chunks (the RIFF is written here around the fixture's streams) read with
    parameters={"decoder": "device"}: iteration across the cache of one batch of 32, seeks backwards, get_frames, and
    get_device_frames into FrameEngine.run_frames"""
    _check_video_file(cases, tmp_path)


@pytest.mark.parametrize("fill", (0xFF, 0xA5), ids=["fill_ff", "fill_a5"])
def test_on_filled_memory_with_guarded_tails(gpu, cases, mixed, encoded, fill, tmp_path, monkeypatch):
    """every case above once more with the test fill mode on: undefined device memory holds the fill byte and every
    buffer, the raw ones of the ABI runs included, has a guarded tail ("Hostile memory")"""
    from video import _hip, ops
    ops.pool_clear()
    _hip.set_fill_mode(fill)
    try:
        _check_valid(cases)
        _check_hostile(cases)
        _check_mixed(mixed)
        _check_forwarding(gpu)
        _check_encoded(encoded)
        for layout in ("420", "422"):
            _check_chunks(gpu, cases, layout, monkeypatch)
        _check_many_frames(cases)
        _check_video_file(cases, tmp_path)
        found = _hip.check_guards()
    finally:
        _hip.set_fill_mode(-1)
        ops.pool_clear()
        _hip.check_guards()
    assert found == [], found
