"""GPU: the 4:2:2 and 4:2:0 encoder (va_jpeg_encode_sampled_u8, ops.jpeg_encode(sampling=...)) and the writer behind
the composer, byte for byte against the pinned streams of DESIGN.md §9, "Subsampled Motion-JPEG encoding"
(tests/jpeg_sampled_encode_checks.py; the fixture tests/golden/mjpeg_encode_sampled_v1.npz holds the small frames and
their bytes, which Pillow decoded when the fixture was written; the large cases are restated here, once).  No
tolerances."""
import os

import numpy as np
import pytest

import jpeg_checks as J
import jpeg_sampled_encode_checks as E
import jpeg_subsampled_checks as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu():
    from video import _hip
    return _hip.lib()


@pytest.fixture(scope="module")
def cases():
    return E.fixture_cases(os.path.join(ROOT, "tests", "golden", "mjpeg_encode_sampled_v1.npz"))[0]


def _same(got, want):
    """np.array_equal on the bytes"""
    return np.array_equal(np.frombuffer(bytes(got), np.uint8), np.frombuffer(bytes(want), np.uint8))


def _check_fixture(cases):
    from video import ops
    seen = 0
    for (shape, hv, quality), group in E.groups(cases).items():
        stack = np.stack([c[3] for c in group])
        got = ops.jpeg_encode(stack, quality, sampling=hv)
        assert len(got) == len(group)
        for c, g in zip(group, got):
            assert _same(g, c[4]), c[0]
            seen += 1
        # frame k of a batch is frame k encoded alone
        alone = ops.jpeg_encode(stack[-1], quality, color=True, sampling={(2, 1): "4:2:2", (2, 2): "4:2:0"}[hv])
        assert len(alone) == 1 and _same(alone[0], got[-1]), (shape, hv, quality)
    assert seen == len(cases) == 356


def test_fixture_cases_equal_the_pinned_bytes(gpu, cases):
    """both layouts x 1x1, 8x8, 16x16, 17x17, 18x34, 9x17, 7x64, 37x53, 80x16, 16x48 and 33x16 x noise, a ramp, all 0
    and all 255 at qualities 1, 50, 90 and 100, and the two checkerboards"""
    _check_fixture(cases)


def test_round_trip_through_the_device_decoder(gpu, cases):
    """ops.jpeg_decode of what ops.jpeg_encode wrote is the restatement's decode of the pinned bytes, status 0"""
    from video import ops
    for hv in ((2, 1), (2, 2)):
        for shape in ((37, 53, 3), (18, 34, 3), (1, 1, 3)):
            group = [c for c in cases if c[1] == hv and c[3].shape == shape and c[2] == 90]
            stack = np.stack([c[3] for c in group])
            frames, status = ops.jpeg_decode(ops.jpeg_encode(stack, 90, sampling=hv), ret_status=True)
            assert not np.asarray(status).any()
            for c, f in zip(group, frames):
                want, st = S.decode(c[4])
                assert st == 0 and np.array_equal(f, want), c[0]


@pytest.fixture(scope="module")
def wide():
    """16 x 16384 at 4:2:0 and 8 x 16384 at 4:2:2, noise at quality 100: one segment of many LDS chunks each"""
    rng = np.random.default_rng(16384)
    out = {}
    for hv, h in (((2, 2), 16), ((2, 1), 8)):
        frame = rng.integers(0, 256, (h, 16384, 3), dtype=np.uint8)
        out[hv] = (frame, S.encode_frame(frame, 100, hv, ri=None))
    return out


@pytest.mark.parametrize("hv", ((2, 2), (2, 1)), ids=["420", "422"])
def test_a_segment_larger_than_any_lds_chunk(gpu, wide, hv):
    from video import ops
    frame, want = wide[hv]
    assert len(want) > 65536 * 3
    got = ops.jpeg_encode(frame, 100, color=True, sampling=hv)
    assert _same(got[0], want)


def test_more_frames_than_a_grid_dimension(gpu, cases):
    """70 000 frames of 16 x 16 at 4:2:0, cycling through the fixture's 16 x 16 cases of quality 90"""
    from video import ops
    group = [c for c in cases if c[1] == (2, 2) and c[3].shape == (16, 16, 3) and c[2] == 90]
    assert len(group) == 4
    n = 70000
    pick = np.arange(n) % len(group)
    stack = np.stack([c[3] for c in group])[pick]
    blob, offsets = ops.jpeg_encode(stack, 90, ret_packed=True, sampling=(2, 2))
    parts = [np.frombuffer(c[4], np.uint8) for c in group]
    assert np.array_equal(np.diff(offsets), np.array([len(p) for p in parts])[pick])
    assert np.array_equal(blob, np.concatenate([parts[k] for k in pick]))


def _abi_run(L, stack, quality, hv, cap, fill=0xA5, c=3):
    """va_jpeg_encode_sampled_u8 on raw buffers filled with `fill`: dict of the downloaded outputs"""
    from video import _hip, ops
    n, h, w = stack.shape[:3]
    tables = ops.jpeg_tables(quality)
    head = np.frombuffer(ops.jpeg_header(h, w, c, quality, hv), np.uint8)
    ins = dict(frames=stack, qt=np.concatenate(tables), head=head)
    dev = {k: _hip.DeviceBuffer.from_array(v) for k, v in ins.items()}
    outs = dict(sizes=(n, np.int64), offsets=(n + 1, np.int64), total=(1, np.int64), out=(max(cap, 1), np.uint8))
    for k, (m, dt) in outs.items():
        dev[k] = _hip.DeviceBuffer(m * np.dtype(dt).itemsize)
        _hip.check(L.va_memset(dev[k].ptr, fill, dev[k].nbytes, None))
    _hip.check(L.va_jpeg_encode_sampled_u8(dev["frames"].ptr, n, h, w, c, hv[0], hv[1], dev["qt"].ptr, dev["head"].ptr,
                                           len(head), dev["sizes"].ptr, dev["offsets"].ptr, dev["total"].ptr,
                                           dev["out"].ptr, cap, None))
    res = {k: dev[k].download((m,), dt) for k, (m, dt) in outs.items()}
    for b in dev.values():
        b.free()
    return res


@pytest.mark.parametrize("hv", ((2, 2), (2, 1)), ids=["420", "422"])
def test_overflow_is_reported_and_nothing_written(gpu, cases, hv):
    group = [c for c in cases if c[1] == hv and c[3].shape == (37, 53, 3) and c[2] == 90]
    stack = np.stack([c[3] for c in group])
    want = [np.frombuffer(c[4], np.uint8) for c in group]
    total = sum(len(w) for w in want)
    offsets = np.concatenate([[0], np.cumsum([len(w) for w in want])])
    short = _abi_run(gpu, stack, 90, hv, total - 1)
    assert short["total"][0] == total and np.array_equal(short["offsets"], offsets)
    assert np.array_equal(short["sizes"], np.diff(offsets))
    assert np.all(short["out"] == 0xA5)                                       # too small by one byte: none written
    full = _abi_run(gpu, stack, 90, hv, total)
    assert full["total"][0] == total and np.array_equal(full["out"], np.concatenate(want))
    assert np.array_equal(full["offsets"], offsets) and np.array_equal(full["sizes"], np.diff(offsets))
    again = _abi_run(gpu, stack, 90, hv, total, fill=0x00)                     # two runs: identical bytes
    for key in full:
        assert full[key].tobytes() == again[key].tobytes(), key
    roomy = _abi_run(gpu, stack, 90, hv, total + 64)
    assert np.array_equal(roomy["out"][:total], full["out"]) and np.all(roomy["out"][total:] == 0xA5)


def test_one_by_one_through_the_new_entry_equals_the_old_one(gpu):
    """(1, 1) runs the instantiations of va_jpeg_encode_u8, in colour and in monochrome"""
    from video import ops
    rng = np.random.default_rng(11)
    for shape in ((3, 37, 53, 3), (3, 37, 53)):
        stack = rng.integers(0, 256, shape, dtype=np.uint8)
        want = J.encode(stack, 90)
        assert [bytes(b) for b in ops.jpeg_encode(stack, 90)] == want
        total = sum(len(b) for b in want)
        got = _abi_run(gpu, stack, 90, (1, 1), total, c=3 if len(shape) == 4 else 1)
        assert got["total"][0] == total and got["out"].tobytes() == b"".join(want)
        assert [bytes(b) for b in ops.jpeg_encode(stack, 90, sampling="4:4:4")] == want


def test_device_frames_in(gpu, cases, monkeypatch):
    from video import ops
    group = [c for c in cases if c[1] == (2, 2) and c[3].shape == (9, 17, 3) and c[2] == 90]
    stack = np.stack([c[3] for c in group])
    dev = ops.DeviceFrames.upload(stack)
    uploads = []
    real = ops._Lease.upload
    monkeypatch.setattr(ops._Lease, "upload", lambda self, arr: uploads.append(arr.nbytes) or real(self, arr))
    try:
        got = ops.jpeg_encode(dev, 90, sampling="4:2:0")
        assert dev.buf is not None and np.array_equal(dev.download(), stack)   # it stays the caller's, untouched
    finally:
        dev.release()
    assert uploads == [128 + 629]                                              # the tables and the header only
    for c, g in zip(group, got):
        assert _same(g, c[4]), c[0]


def test_retry_with_exact_room(gpu, cases):
    """noise at quality 100 needs more than the first launch's room: the second launch writes the same bytes"""
    from video import ops
    case = [c for c in cases if c[0] == "noise_37x53_q100_420"][0]
    assert 3 * len(case[4]) > 3 * (629 + 2 * 3) + 3 * case[3].size // ops.JPEG_ROOM_DIVISOR
    assert all(_same(g, case[4]) for g in ops.jpeg_encode(np.stack([case[3]] * 3), 100, sampling=(2, 2)))


@pytest.mark.parametrize("fill", (0xFF, 0xA5), ids=["fill_ff", "fill_a5"])
def test_on_filled_memory_with_guarded_tails(gpu, cases, wide, fill):
    """every case again with the test fill mode on: undefined device memory holds the fill byte and every buffer
    has a guarded tail ("Hostile memory")"""
    from video import _hip, ops
    ops.pool_clear()
    _hip.set_fill_mode(fill)
    try:
        for _ in (1, 2):                                                       # the second round gets recycled buffers
            _check_fixture(cases)
        for hv in ((2, 2), (2, 1)):
            assert _same(ops.jpeg_encode(wide[hv][0], 100, color=True, sampling=hv)[0], wide[hv][1])
        case = [c for c in cases if c[0] == "noise_37x53_q100_420"][0]
        assert all(_same(g, case[4]) for g in ops.jpeg_encode(np.stack([case[3]] * 3), 100, sampling=(2, 2)))   # the retry
        found = _hip.check_guards()
    finally:
        _hip.set_fill_mode(-1)
        ops.pool_clear()
        _hip.check_guards()
    assert found == [], found


def test_composer_writes_a_420_clip_that_the_device_decoder_reads(gpu, tmp_path):
    """5 frames of 37 x 53 through VideoComposer("x.avi", sampling="4:2:0") and back through the device decoder: the
    frames are the restatement's decode of the restatement's bytes for the composed frames"""
    from video.io.backend_mjpeg import VideoMJPEG
    from video.io.composer import VideoComposer
    rng = np.random.default_rng(5)
    h, w = 37, 53
    frames = rng.integers(0, 200, (5, h, w, 3), dtype=np.uint8)

    def compose(sink, **kwargs):
        vc = VideoComposer(sink, (w, h), 25, True, **kwargs)
        for f in frames:
            vc.set_frame(f)
            vc.add_circle((30, 20), 9, "r", thickness=1)
            vc.add_rectangle((5, 6, 40, 30), "w")
        vc.close()
        return vc
    composed = compose(None).frames
    path = str(tmp_path / "x.avi")
    assert compose(path, quality=80, sampling="4:2:0").frames_written == 5
    want = E.encode(composed, 80, (2, 2))
    with VideoMJPEG(path, {"decoder": "device"}) as video:
        assert video.frame_count == 5 and video.size == (w, h) and video.is_color
        for k in range(5):
            assert _same(video.get_frame_bytes(k), want[k]), k
            assert np.array_equal(video.get_frame(k), S.decode(want[k])[0]), k
    J.parse_avi(open(path, "rb").read())
