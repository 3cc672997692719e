"""GPU: the batched JPEG decoder (va_jpeg_decode_u8, ops.jpeg_decode), VideoMJPEG's device decoder and
FrameEngine.run_frames, byte for byte against the NumPy restatement tests/jpeg_decode_checks.py (DESIGN.md §9,
"Motion-JPEG decoding").  The fixture tests/golden/mjpeg_decode_v1.npz holds the restatement's pixels and status
words of the small streams; the large cases are restated here, once.  No tolerances."""
import os

import numpy as np
import pytest

import jpeg_checks as J
import jpeg_decode_checks as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plus(pillow, difference):
    """the fixture stores the expected pixels as their int8 difference from Pillow's decode of the same stream"""
    return (pillow.astype(np.int16) + difference).astype(np.uint8)


@pytest.fixture(scope="module")
def gpu():
    from video import _hip
    return _hip.lib()


def _hostile_pixels(enc, dec, name):
    """(c) stores pixels as their difference modulo 256 from those of the intact stream the case was made from"""
    source = name.rsplit("_", 2)[0] if "_cut_" in name or "_rst_" in name or "_no_eoi" in name else name.rsplit("_", 1)[0]
    return _plus(enc["pillow_" + source], dec["a_dpx_" + source]) + dec["c_dpx_" + name]


@pytest.fixture(scope="module")
def cases():
    """{'a' | 'b' | 'c': [(name, bytes, expected pixels, expected status)]} of the fixture"""
    enc = np.load(os.path.join(ROOT, "tests", "golden", "mjpeg_v1.npz"), allow_pickle=False)
    dec = np.load(os.path.join(ROOT, "tests", "golden", "mjpeg_decode_v1.npz"), allow_pickle=False)
    out = {"a": [(str(n), enc["bytes_" + n].tobytes(), _plus(enc["pillow_" + n], dec["a_dpx_" + n]), 0)
                 for n in dec["names_a"]],
           "b": [(str(n), dec["b_bytes_" + n].tobytes(), _plus(dec["b_pillow_" + n.rsplit("_", 1)[0]], dec["b_dpx_" + n.rsplit("_", 1)[0]]), 0) for n in dec["names_b"]],
           "c": [(str(n), dec["c_bytes_" + n].tobytes(), _hostile_pixels(enc, dec, n), int(s))
                 for n, s in zip(dec["names_c"], dec["status_c"])]}
    assert (len(out["a"]), len(out["b"]), len(out["c"])) == (120, 96, 28)
    return out


def _by_header(items):
    """the cases grouped into batches of one header: [[case]]"""
    groups = {}
    for item in items:
        groups.setdefault(D.header_key(D.parse_header(item[1])), []).append(item)
    return list(groups.values())


def _check_valid(cases):
    from video import ops
    seen = 0
    for batch in _by_header(cases["a"] + cases["b"]):
        got, status = ops.jpeg_decode([data for _, data, _, _ in batch], ret_status=True)
        assert got.dtype == np.uint8 and len(got) == len(batch) and not status.any(), batch[0][0]
        for (name, _, want, _), g in zip(batch, got):
            assert np.array_equal(g, want), name
            seen += 1
        alone = ops.jpeg_decode([batch[-1][1]])                      # frame k of a batch is frame k decoded alone
        assert alone.shape == (1,) + batch[-1][2].shape and np.array_equal(alone[0], batch[-1][2]), batch[-1][0]
    assert seen == 216


def _check_hostile(cases):
    from video import ops
    for name, data, want, want_status in cases["c"]:
        got, status = ops.jpeg_decode([data], ret_status=True)
        assert status.dtype == np.int32 and status[0] == want_status, (name, status, want_status)
        assert np.array_equal(got[0], want), name
        if want_status:
            with pytest.raises(ValueError) as err:
                ops.jpeg_decode([data])
            assert "frame 0" in str(err.value) and ops.jpeg_status_text(want_status) in str(err.value)
        else:
            assert np.array_equal(ops.jpeg_decode([data])[0], want)
    # a hostile frame between two good ones of its header changes neither of them
    mono = [c for c in cases["c"] if "x1_" in c[0]]
    good = [c for c in cases["a"] if c[0] == "noise_q50_37x53x1"][0]
    batch = [good] + mono + [good]
    got, status = ops.jpeg_decode([c[1] for c in batch], ret_status=True)
    assert status.tolist() == [c[3] for c in batch]
    assert all(np.array_equal(g, c[2]) for g, c in zip(got, batch))


def test_valid_fixture_streams_equal_the_restatement(gpu, cases):
    """the encoder's own 120 streams and 96 Pillow-written ones: no restart markers, one per MCU row, one every 3
    blocks (segments cross MCU rows, the last is short), optimised Huffman tables"""
    _check_valid(cases)


def test_hostile_streams_equal_the_restatement(gpu, cases):
    assert {s for _, _, _, s in cases["c"]} >= {0, 1, 2, 8, 12}
    _check_hostile(cases)


def _strip_restarts(data):
    """the stream without its DRI segment and without its RST markers: one segment"""
    head = D.parse_header(data)
    dri = data.index(b"\xff\xdd\x00\x04")
    assert dri < head["scan_begin"]
    segs, bit = D.split_segments(data, head["scan_begin"], head["nseg"])
    assert bit == 0
    body = b"".join(data[b:e] for b, e in segs)
    return data[:dri] + data[dri + 6:head["scan_begin"]] + body + b"\xff\xd9"


@pytest.fixture(scope="module")
def wide():
    """8 x 16384 noise at quality 100, as the encoder's restatement writes it (one segment of 2048 MCUs, with DRI)
    and without DRI and restart markers; the restatement's decode of each: {c: [frame, (bytes, pixels) * 2]}"""
    rng = np.random.default_rng(16384)
    out = {}
    for c in (1, 3):
        frame = rng.integers(0, 256, (8, 16384) + ((3,) if c == 3 else ()), dtype=np.uint8)
        data = J.encode_frame(frame, 100)
        bare = _strip_restarts(data)
        assert D.parse_header(bare)["nseg"] == 1 and D.parse_header(bare)["ri"] == 2048
        out[c] = [frame]
        for stream in (data, bare):
            pixels, status = D.decode(stream)
            assert status == 0
            out[c].append((stream, pixels))
        assert np.array_equal(out[c][1][1], out[c][2][1])
    return out


def _check_wide(wide, c):
    """the frame encoded by ops.jpeg_encode (one row of 2048 MCUs per segment), and that stream with DRI and the
    restart markers stripped on the host (one segment of 2048 MCUs)"""
    from video import ops
    frame, (data, want), (bare, want_bare) = wide[c]
    encoded = ops.jpeg_encode(frame, 100, color=c == 3)[0]
    assert encoded == data
    assert np.array_equal(ops.jpeg_decode([encoded], color=c == 3)[0], want)
    assert _strip_restarts(encoded) == bare
    assert np.array_equal(ops.jpeg_decode([bare], color=c == 3)[0], want_bare)


@pytest.mark.parametrize("c", (1, 3))
def test_one_long_row_with_and_without_restart_markers(gpu, wide, c):
    _check_wide(wide, c)


def _check_many_frames(cases):
    from video import ops
    picks = [c for c in cases["a"] if c[0].endswith("_8x8x1")]
    groups = _by_header(picks)
    distinct = max(groups, key=len)
    assert len(distinct) >= 4
    n = 70000
    pick = np.arange(n) % len(distinct)
    parts = [np.frombuffer(c[1], np.uint8) for c in distinct]
    sizes = np.array([len(p) for p in parts])[pick]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    blob = np.concatenate(parts * (n // len(parts) + 1))[:offsets[-1]]
    got = ops.jpeg_decode((blob, offsets))
    assert got.shape == (n, 8, 8)
    assert np.array_equal(got, np.stack([c[2] for c in distinct])[pick])


def test_more_frames_than_a_grid_dimension(gpu, cases):
    """70 000 frames of 8 x 8, cycling through the fixture's 8 x 8 monochrome streams of quality 90"""
    _check_many_frames(cases)


def _abi_run(L, batch, workspace_bytes=None, fill=0xA5, extra=0):
    """va_jpeg_decode_u8 on raw buffers filled with `fill`: (pixels with `extra` bytes behind them, status)"""
    from video import _hip, ops
    heads = [ops.jpeg_parse_header(data) for data in batch]
    head = heads[0]
    n, h, w, c, ri = len(batch), head["h"], head["w"], head["c"], head["ri"]
    tables = b"".join(ops._jpeg_decode_table(*dc) + ops._jpeg_decode_table(*ac) for dc, ac in head["huff"])
    offsets = np.concatenate([[0], np.cumsum([len(d) for d in batch])]).astype(np.int64)
    ins = dict(bytes=np.frombuffer(b"".join(batch), np.uint8), offsets=offsets,
               scan=np.array([hd["scan_begin"] for hd in heads], np.int64), qt=head["qtables"].ravel(),
               huff=np.frombuffer(tables, np.uint8))
    dev = {k: _hip.DeviceBuffer.from_array(v) for k, v in ins.items()}
    full = int(L.va_jpeg_decode_workspace_bytes(n, h, w, c, ri))
    room = full if workspace_bytes is None else workspace_bytes
    outs = dict(out=(n * h * w * c + extra, np.uint8), status=(n, np.int32), ws=(room, np.uint8))
    for k, (m, dt) in outs.items():
        dev[k] = _hip.DeviceBuffer(m * np.dtype(dt).itemsize)
        _hip.check(L.va_memset(dev[k].ptr, fill, dev[k].nbytes, None))
    try:
        _hip.check(L.va_jpeg_decode_u8(dev["bytes"].ptr, dev["offsets"].ptr, dev["scan"].ptr, n, h, w, c, ri,
                                       dev["qt"].ptr, dev["huff"].ptr, len(tables), dev["out"].ptr, dev["status"].ptr,
                                       dev["ws"].ptr, room, None))
        return dev["out"].download((outs["out"][0],), np.uint8), dev["status"].download((n,), np.int32)
    finally:
        for b in dev.values():
            b.free()


def _check_chunks(gpu, cases, c, monkeypatch):
    valid = [x for x in cases["a"] if x[0].endswith("_37x53x%d" % c)]
    source = "noise_q50_37x53x1" if c == 1 else "noise_q90_37x53x3"
    key = D.header_key(D.parse_header([x for x in valid if x[0] == source][0][1]))
    same = [x for x in valid if D.header_key(D.parse_header(x[1])) == key]
    hostile = [x for x in cases["c"] if x[0].startswith(source)]
    batch = (same + hostile)[:8]
    assert len(batch) == 8 and any(x[3] for x in batch)
    data = [x[1] for x in batch]
    want = np.concatenate([x[2].ravel() for x in batch])
    pixels, status = _abi_run(gpu, data, extra=64)
    assert np.array_equal(pixels[:-64], want) and np.all(pixels[-64:] == 0xA5)
    assert status.tolist() == [x[3] for x in batch]
    three = int(gpu.va_jpeg_decode_workspace_bytes(3, 37, 53, c, 7))
    assert three * 2 < int(gpu.va_jpeg_decode_workspace_bytes(8, 37, 53, c, 7))
    chunked = _abi_run(gpu, data, workspace_bytes=three, fill=0x00, extra=64)
    assert np.array_equal(chunked[0][:-64], pixels[:-64]) and np.array_equal(chunked[1], status)
    assert not chunked[0][-64:].any()
    again = _abi_run(gpu, data, extra=64)
    assert again[0].tobytes() == pixels.tobytes() and again[1].tobytes() == status.tobytes()
    from video import _hip
    one = int(gpu.va_jpeg_decode_workspace_bytes(1, 37, 53, c, 7))
    with pytest.raises(_hip.HipError) as err:                       # VA_ERR_RANGE: not even one frame fits
        _abi_run(gpu, data, workspace_bytes=one - 256)
    assert err.value.code == -34 and "one frame" in str(err.value)
    # the same through ops.jpeg_decode's own (pooled) workspace, capped at what 3 frames need
    from video import ops
    asked = []

    class Counting(object):
        def __getattr__(self, name):
            fn = getattr(gpu, name)
            if name != "va_jpeg_decode_u8":
                return fn

            def counted(*args):
                asked.append((args[3], args[14]))
                return fn(*args)
            return counted
    with monkeypatch.context() as patch:
        patch.setattr(ops, "JPEG_DECODE_WORKSPACE_MAX", three)
        patch.setattr(_hip, "lib", lambda device=None: Counting())
        got, got_status = ops.jpeg_decode(data, ret_status=True)
    assert asked == [(8, three)]
    assert np.array_equal(got.ravel(), want) and got_status.tolist() == [x[3] for x in batch]


@pytest.mark.parametrize("c", (1, 3))
def test_chunks_two_runs_and_a_roomy_buffer(gpu, cases, c, monkeypatch):
    """a workspace that holds 3 of 8 frames (three chunks) gives the bytes of the single-chunk run, at the ABI and
    through ops.jpeg_decode with its workspace cap lowered; two runs write identical bytes; the bytes behind the
    last frame stay as they were.  Hostile frames ride along."""
    _check_chunks(gpu, cases, c, monkeypatch)


def _check_round_trip(cases, monkeypatch):
    from video import ops
    rng = np.random.default_rng(11)
    stack = rng.integers(0, 256, (5, 37, 53, 3), dtype=np.uint8)
    dev = ops.DeviceFrames.upload(stack)
    uploads = []
    real = ops._Lease.upload
    monkeypatch.setattr(ops._Lease, "upload", lambda self, arr: uploads.append(arr.nbytes) or real(self, arr))
    try:
        blob, offsets = ops.jpeg_encode(dev, 90, ret_packed=True)
        del uploads[:]
        back = ops.jpeg_decode((blob, offsets), keep=True)
        try:
            assert isinstance(back, ops.DeviceFrames) and back.shape == stack.shape
            got = back.download()
        finally:
            back.release()
    finally:
        dev.release()
    tables = 3 * 64 + 6 * ops.JPEG_HUFF_DECODE_BYTES
    assert uploads == [len(blob), 8 * (5 + 1 + 5), tables] and len(blob) < stack.nbytes
    for k in range(5):
        data = blob[offsets[k]:offsets[k + 1]].tobytes()
        assert data == J.encode_frame(stack[k], 90)
        assert np.array_equal(got[k], D.decode(data)[0]), k
    mixed = [cases["a"][0][1], [c for c in cases["a"] if c[0].endswith("37x53x1")][0][1]]
    with pytest.raises(ValueError):
        ops.jpeg_decode(mixed)                                          # mixed shapes
    with pytest.raises(ValueError):
        ops.jpeg_decode([cases["a"][0][1]], color=cases["a"][0][2].ndim == 2)
    assert ops.jpeg_decode([]).shape == (0, 0, 0)


def test_round_trip_on_the_device(gpu, cases, monkeypatch):
    """DeviceFrames -> jpeg_encode(ret_packed=True) -> jpeg_decode(keep=True): the restatement's decode of those
    bytes, and no pixel is uploaded"""
    with monkeypatch.context() as patch:
        _check_round_trip(cases, patch)


@pytest.mark.parametrize("fill", (0xFF, 0xA5), ids=["fill_ff", "fill_a5"])
def test_on_filled_memory_with_guarded_tails(gpu, cases, wide, fill, tmp_path, monkeypatch):
    """every case above again with the test fill mode on: undefined device memory holds the fill byte and every
    buffer, the raw ones of the ABI runs included, has a guarded tail ("Hostile memory")"""
    from video import _hip, ops
    ops.pool_clear()
    _hip.set_fill_mode(fill)
    try:
        for _ in (1, 2):                                                       # the second round gets recycled buffers
            _check_valid(cases)
            _check_hostile(cases)
        for c in (1, 3):
            _check_wide(wide, c)
            _check_chunks(gpu, cases, c, monkeypatch)
        _check_many_frames(cases)
        with monkeypatch.context() as patch:
            _check_round_trip(cases, patch)
        _check_video_file(tmp_path)
        _check_engine()
        found = _hip.check_guards()
    finally:
        _hip.set_fill_mode(-1)
        ops.pool_clear()
        _hip.check_guards()
    assert found == [], found


def test_video_file_with_the_device_decoder(gpu, tmp_path):
    """a 70-frame 37 x 53 file written by VideoWriterMJPEG, read with parameters={"decoder": "device"}: iteration,
    indexing, negative indices, get_frames and get_device_frames; the cache of one batch of 32 is crossed twice and
    seeked backwards"""
    _check_video_file(tmp_path)


def _check_video_file(tmp_path):
    from video import ops
    from video.io.backend_mjpeg import VideoMJPEG, VideoWriterMJPEG
    from video.io.file import load_any_video
    rng = np.random.default_rng(70)
    frames = rng.integers(0, 256, (70, 37, 53, 3), dtype=np.uint8)
    path = str(tmp_path / "clip.avi")
    with VideoWriterMJPEG(path, size=(53, 37), fps=25, is_color=True, quality=85) as writer:
        for f in frames:
            writer.write_frame(f)
    calls = []
    real = ops.jpeg_decode
    with VideoMJPEG(path) as plain:
        want = np.stack([D.decode(plain.get_frame_bytes(k))[0] for k in range(70)])
    video = load_any_video(path, {"decoder": "device"})
    try:
        ops.jpeg_decode = lambda streams, **kw: calls.append(len(streams)) or real(streams, **kw)
        assert video.frame_count == 70 and VideoMJPEG.DEVICE_BATCH == 32
        got = np.stack([f for f in video])
        assert np.array_equal(got, want) and calls == [32, 32, 6]
        del calls[:]
        for k in (69, 3, 40, 41, -1, -70, 31, 32):
            assert np.array_equal(video[k], want[k]), k
        assert calls == [32, 32, 6, 32, 32]
        del calls[:]
        assert np.array_equal(video.get_frames(10, 45), want[10:45]) and calls == [35]
        dev = video.get_device_frames(60, None)
        try:
            assert isinstance(dev, ops.DeviceFrames) and dev.shape == (10, 37, 53, 3)
            assert np.array_equal(dev.download(), want[60:])
        finally:
            dev.release()
        with pytest.raises(IndexError):
            video.get_frame(70)
        with pytest.raises(IndexError):
            video.get_frames(5, 71)
    finally:
        ops.jpeg_decode = real
        video.close()
    with pytest.raises(ValueError):
        VideoMJPEG(path, {"decoder": "ffmpeg"})


def test_engine_runs_on_decoded_device_frames(gpu):
    """FrameEngine.run_frames on the decoded stack equals run() on its download"""
    _check_engine()


def _check_engine():
    from video import ops
    from video.engine import FrameEngine
    yy, xx = np.mgrid[:48, :64]
    frames = np.stack([np.where((yy - 24) ** 2 + (xx - 20 - 3 * k) ** 2 < 100, 220, 30).astype(np.uint8)
                       for k in range(6)])
    streams = ops.jpeg_encode(frames, 90)
    dev = ops.jpeg_decode(streams, keep=True)
    try:
        host = dev.download()
        assert np.array_equal(host, np.stack([D.decode(s)[0] for s in streams]))
        kw = dict(size=(64, 48), channels=1, max_batch=8, sigma=1.0, thresh=100, connectivity=8, max_labels=16)
        want = FrameEngine(**kw).run(host, want=("filtered", "mask", "labels", "counts"))
        got = FrameEngine(**kw).run_frames(dev, want=("filtered", "mask", "labels", "counts"))
        assert sorted(got) == sorted(want) and want["counts"].min() >= 1
        for key in want:
            assert np.array_equal(got[key], want[key]), key
        assert np.array_equal(dev.download(), host)                         # the stack stays the caller's, untouched
    finally:
        dev.release()
