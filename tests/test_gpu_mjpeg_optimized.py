"""GPU: Motion-JPEG with Huffman tables made for the call (va_jpeg_encode_optimized_u8, va_jpeg_optimal_tables,
ops.jpeg_encode(optimize=True), ops.jpeg_optimal_tables, VideoWriterMJPEG(optimize=True)), byte for byte against the
definition of DESIGN.md §9, "Optimised Huffman tables" (tests/jpeg_optimize_checks.py) and the fixture
tests/golden/mjpeg_optimized_v1.npz: libjpeg's own tables for the counts of files Pillow wrote, chosen counts, and
small calls whose streams Pillow decoded when the fixture was written.  The restatement's streams are computed once
per case and shared.  No tolerances."""
import os

import numpy as np
import pytest

import jpeg_checks as J
import jpeg_optimize_checks as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLING = dict(O.LAYOUTS)


@pytest.fixture(scope="module")
def gpu():
    from video import _hip
    return _hip.lib()


@pytest.fixture(scope="module")
def fx():
    return O.fixture(os.path.join(ROOT, "tests", "golden", "mjpeg_optimized_v1.npz"))[0]


_WANT = {}


def _case(layout, n, h, w, quality):
    """(the stack, the restatement's files, its tables): computed once, left unchanged"""
    key = (layout, n, h, w, quality)
    if key not in _WANT:
        stack = O.stack_of(n, h, w, 1 if layout == "mono" else 3, 1000 * h + w)
        _WANT[key] = (stack,) + O.encode(stack, quality, SAMPLING[layout])
    return _WANT[key]


def _encode(stack, quality, layout, **kwargs):
    from video import ops
    return ops.jpeg_encode(stack, quality, sampling=SAMPLING[layout] or (1, 1), optimize=True, **kwargs)


def _same_files(got, want, where):
    assert len(got) == len(want), where
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(np.frombuffer(bytes(g), np.uint8), np.frombuffer(w, np.uint8)), (where, k)


# ------------------------------------------------------------------------------------------------ the table kernel
def test_table_kernel_on_libjpeg_s_tables_and_on_chosen_counts(gpu, fx):
    """fixture parts 1 and 2 in one call: 240 tables of files Pillow wrote with optimize=True, then one and two
    symbols, 256 equal counts, 256 ones, a DC shape, Fibonacci counts (sizes beyond 16 before the limit), powers of
    two (sizes beyond 32) and 200 random tables with zeros"""
    from video import ops
    counts = np.concatenate([c for _, c, _ in fx["pin"]] + [c[None] for _, c, _ in fx["chosen"]])
    want = np.concatenate([t for _, _, t in fx["pin"]] + [t[None] for _, _, t in fx["chosen"]])
    assert len(counts) == 240 + 207 and counts.dtype == np.int64
    got = ops.jpeg_optimal_tables(counts)
    assert got.dtype == np.uint8 and got.shape == want.shape
    wrong = np.flatnonzero((got != want).any(axis=1))
    assert len(wrong) == 0, wrong[:10]
    one = ops.jpeg_optimal_tables(counts[7])
    assert one.shape == (O.TABLE_BYTES,) and np.array_equal(one, want[7])
    assert np.array_equal(ops.jpeg_optimal_tables(counts[:5].astype(np.uint32)), want[:5])      # 5: not a multiple of 4 waves
    assert not ops.jpeg_optimal_tables(np.zeros(256, np.int64)).any()
    assert ops.jpeg_optimal_tables(np.zeros((0, 256), np.int64)).shape == (0, O.TABLE_BYTES)
    assert np.array_equal(ops.jpeg_optimal_tables(counts), got)                                 # two runs


# ------------------------------------------------------------------------------------------------ the encoder
def test_fixture_calls_equal_the_stored_bytes(gpu, fx):
    """the streams that Pillow decoded when the fixture was written"""
    assert len(fx["calls"]) == 20
    for name, layout, quality, frames, files, tables, _ in fx["calls"]:
        got, got_tables = _encode(frames, quality, layout, ret_tables=True)
        _same_files(got, files, name)
        assert np.array_equal(got_tables, tables), name


@pytest.mark.parametrize("layout", [name for name, _ in O.LAYOUTS])
def test_shapes_qualities_and_batches_equal_the_restatement(gpu, layout):
    """1x1, 8x8, 7x9, 16x16, 17x33, 37x53 and a row of more than one chunk per segment, at qualities 1, 50, 90 and 100,
    as one noise frame and as a constant-0 frame, a noise frame and a ramp in one call: the tables are those of the
    sum of the three, which differ from every single frame's"""
    for h, w in O.SHAPES + (O.WIDE[layout],):
        for quality in O.QUALITIES:
            for n in (1, 3):
                stack, files, tables = _case(layout, n, h, w, quality)
                got, got_tables = _encode(stack, quality, layout, ret_tables=True)
                _same_files(got, files, (layout, h, w, quality, n))
                assert np.array_equal(got_tables, tables), (layout, h, w, quality, n)
    stack, files, tables = _case(layout, 3, 37, 53, 90)
    for k in range(3):
        alone = O.encode(stack[k:k + 1], 90, SAMPLING[layout])
        assert not np.array_equal(alone[1], tables) and alone[0][0] != files[k]


def test_a_string_of_more_than_64_bits(gpu):
    """a coefficient behind a run of 62 under a ZRL code of 16 bits adds 69 bits (at most 3 * 16 + 16 + 10 = 74 with
    tables made on the device): the kernels emit the ZRLs as a string of their own"""
    from video import ops
    stack = O.long_run_stack()
    files, tables = O.encode(stack, 90, None)
    assert O.long_run_bits(stack, 90, tables) == (16, 69)
    got, got_tables = _encode(stack, 90, "mono", ret_tables=True)
    assert np.array_equal(got_tables, tables)
    _same_files(got, files, "long run")
    a, sa = ops.jpeg_decode(got, ret_status=True)
    b, sb = ops.jpeg_decode(ops.jpeg_encode(stack, 90), ret_status=True)
    assert not np.asarray(sa).any() and not np.asarray(sb).any() and np.array_equal(np.asarray(a), np.asarray(b))


def test_device_frames_in_and_packed_out(gpu, monkeypatch):
    from video import ops
    stack, files, tables = _case("420", 3, 17, 33, 90)
    dev = ops.DeviceFrames.upload(stack)
    uploads = []
    real = ops._Lease.upload
    monkeypatch.setattr(ops._Lease, "upload", lambda self, arr: uploads.append(arr.nbytes) or real(self, arr))
    try:
        (blob, offsets), got_tables = _encode(dev, 90, "420", ret_packed=True, ret_tables=True)
        assert dev.buf is not None and np.array_equal(dev.download(), stack)
    finally:
        dev.release()
    pre, post = ops.jpeg_header_pieces(ops.jpeg_header(17, 33, 3, 90, (2, 2)))
    assert uploads == [128 + len(pre) + len(post)]                  # one upload: the quantisation tables and the header
    assert np.array_equal(np.diff(offsets), [len(f) for f in files]) and blob.tobytes() == b"".join(files)
    assert np.array_equal(got_tables, tables)


@pytest.mark.parametrize("layout", [name for name, _ in O.LAYOUTS])
def test_device_decoder_reads_the_same_frames_as_from_the_plain_stream(gpu, layout):
    from video import ops
    stack, files, _ = _case(layout, 3, 37, 53, 90)
    plain = ops.jpeg_encode(stack, 90, sampling=SAMPLING[layout] or (1, 1))
    optimised = _encode(stack, 90, layout)
    assert sum(map(len, optimised)) < sum(map(len, plain))
    a, sa = ops.jpeg_decode(optimised, ret_status=True)
    b, sb = ops.jpeg_decode(plain, ret_status=True)
    assert not np.asarray(sa).any() and not np.asarray(sb).any()
    assert np.array_equal(np.asarray(a), np.asarray(b))
    assert ops.jpeg_decode_groups([ops.jpeg_parse_header(f, "any") for f in optimised]) == [(0, 3)]


def test_retry_with_exact_room(gpu):
    """noise at quality 100 needs more than the first launch's room: the second launch writes the same bytes"""
    from video import ops
    stack, files, _ = _case("444", 1, 37, 53, 100)
    assert len(files[0]) > len(ops.jpeg_header(37, 53, 3, 100)) + 2 * 5 + stack.size // ops.JPEG_ROOM_DIVISOR
    _same_files(_encode(stack, 100, "444"), files, "retry")


# ------------------------------------------------------------------------------------------------ the C ABI
def _abi_run(L, stack, quality, layout, cap, fill=0xA5):
    """va_jpeg_encode_optimized_u8 on raw buffers filled with `fill`: dict of the downloaded outputs"""
    from video import _hip, ops
    n, h, w = stack.shape[:3]
    c = 1 if stack.ndim == 3 else 3
    hv = SAMPLING[layout] or (1, 1)
    pre, post = ops.jpeg_header_pieces(ops.jpeg_header(h, w, c, quality, hv))
    ins = dict(frames=stack, qt=np.concatenate(ops.jpeg_tables(quality)), pre=np.frombuffer(pre, np.uint8),
               post=np.frombuffer(post, np.uint8))
    dev = {k: _hip.DeviceBuffer.from_array(v) for k, v in ins.items()}
    outs = dict(sizes=(n, np.int64), offsets=(n + 1, np.int64), total=(1, np.int64), out=(max(cap, 1), np.uint8),
                tables=((2 if c == 1 else 4) * O.TABLE_BYTES, np.uint8))
    for k, (m, dt) in outs.items():
        dev[k] = _hip.DeviceBuffer(m * np.dtype(dt).itemsize)
        _hip.check(L.va_memset(dev[k].ptr, fill, dev[k].nbytes, None))
    _hip.check(L.va_jpeg_encode_optimized_u8(dev["frames"].ptr, n, h, w, c, hv[0], hv[1], dev["qt"].ptr, dev["pre"].ptr,
                                             len(pre), dev["post"].ptr, len(post), dev["tables"].ptr, dev["sizes"].ptr,
                                             dev["offsets"].ptr, dev["total"].ptr, dev["out"].ptr, cap, None))
    res = {k: dev[k].download((m,), dt) for k, (m, dt) in outs.items()}
    for b in dev.values():
        b.free()
    return res


@pytest.mark.parametrize("layout", ("mono", "420"))
def test_overflow_is_reported_and_nothing_written(gpu, layout):
    stack, files, tables = _case(layout, 3, 37, 53, 90)
    want = [np.frombuffer(f, np.uint8) for f in files]
    total = sum(len(w) for w in want)
    offsets = np.concatenate([[0], np.cumsum([len(w) for w in want])])
    short = _abi_run(gpu, stack, 90, layout, total - 1)
    assert short["total"][0] == total and np.array_equal(short["offsets"], offsets)
    assert np.array_equal(short["sizes"], np.diff(offsets))
    assert np.all(short["out"] == 0xA5)                                       # too small by one byte: none written
    assert np.array_equal(short["tables"], tables.ravel())
    full = _abi_run(gpu, stack, 90, layout, total)
    assert full["total"][0] == total and np.array_equal(full["out"], np.concatenate(want))
    assert np.array_equal(full["offsets"], offsets) and np.array_equal(full["sizes"], np.diff(offsets))
    again = _abi_run(gpu, stack, 90, layout, total, fill=0x00)                 # two runs: identical bytes
    for key in full:
        assert full[key].tobytes() == again[key].tobytes(), key
    roomy = _abi_run(gpu, stack, 90, layout, total + 64, fill=0xFF)
    assert np.array_equal(roomy["out"][:total], full["out"]) and np.all(roomy["out"][total:] == 0xFF)


def test_no_frames_enqueue_nothing(gpu):
    from video import _hip, ops
    buf = _hip.DeviceBuffer(64)
    _hip.check(gpu.va_memset(buf.ptr, 0x5A, 64, None))
    assert gpu.va_jpeg_encode_optimized_u8(None, 0, 8, 8, 3, 2, 2, None, None, 1, None, 1, buf.ptr, buf.ptr, buf.ptr,
                                           buf.ptr, buf.ptr, 64, None) == 0
    assert gpu.va_jpeg_optimal_tables(None, 0, buf.ptr, None) == 0
    assert np.all(buf.download((64,), np.uint8) == 0x5A)
    buf.free()
    assert ops.jpeg_encode(np.zeros((0, 8, 8, 3), np.uint8), optimize=True) == []
    files, tables = ops.jpeg_encode(np.zeros((0, 8, 8), np.uint8), optimize=True, ret_tables=True)
    assert files == [] and tables.shape == (2, O.TABLE_BYTES) and not tables.any()


@pytest.mark.parametrize("fill", (0xFF, 0xA5), ids=["fill_ff", "fill_a5"])
def test_on_filled_memory_with_guarded_tails(gpu, fx, fill):
    """the test fill mode ("Hostile memory"): undefined device memory, the library's scratch with the counts
    in it included, holds the fill byte, and every buffer has a guarded tail; two rounds, the second on recycled buffers"""
    from video import _hip, ops
    counts = np.concatenate([c for _, c, _ in fx["pin"][:6]] + [c[None] for _, c, _ in fx["chosen"][:9]])
    want = np.concatenate([t for _, _, t in fx["pin"][:6]] + [t[None] for _, _, t in fx["chosen"][:9]])
    ops.pool_clear()
    _hip.set_fill_mode(fill)
    try:
        for _ in (1, 2):
            for layout, _ in O.LAYOUTS:
                for h, w in ((1, 1), (7, 9), (37, 53), O.WIDE[layout]):
                    stack, files, tables = _case(layout, 3, h, w, 90)
                    got, got_tables = _encode(stack, 90, layout, ret_tables=True)
                    _same_files(got, files, (layout, h, w))
                    assert np.array_equal(got_tables, tables), (layout, h, w)
            stack, files, _ = _case("444", 1, 37, 53, 100)
            _same_files(_encode(stack, 100, "444"), files, "retry")
            assert np.array_equal(ops.jpeg_optimal_tables(counts), want)
        found = _hip.check_guards()
    finally:
        _hip.set_fill_mode(-1)
        ops.pool_clear()
        _hip.check_guards()
    assert found == [], found


# ------------------------------------------------------------------------------------------------ the writer
def test_writer_writes_runs_of_its_batch_that_both_decoders_read(gpu, tmp_path):
    """40 frames of 37 x 53 at 4:2:0 with batch=16: runs of 16, 16 and 8 frames with one header each, the bytes of three
    optimised calls; Pillow and the device decoder read what they read from the plain file"""
    from video import ops
    from video.io.backend_mjpeg import VideoMJPEG, VideoWriterMJPEG
    rng = np.random.default_rng(40)
    yy, xx = np.mgrid[:37, :53]
    clip = np.stack([np.stack([(xx * 4 + 5 * t) % 256, (yy * 6 + t) % 256, rng.integers(0, 40 + 5 * t, (37, 53))], axis=-1)
                     for t in range(40)]).astype(np.uint8)
    paths = {flag: str(tmp_path / ("%s.avi" % flag)) for flag in (False, True)}
    for flag, path in paths.items():
        with VideoWriterMJPEG(path, (53, 37), 25, quality=85, batch=16, sampling="4:2:0", optimize=flag) as writer:
            for f in clip:
                writer.write_frame(f)
    want = sum((O.encode(clip[a:b], 85, (2, 2))[0] for a, b in ((0, 16), (16, 32), (32, 40))), [])
    J.parse_avi(open(paths[True], "rb").read())
    assert os.path.getsize(paths[True]) < os.path.getsize(paths[False])
    with VideoMJPEG(paths[True]) as video:
        stored = [video.get_frame_bytes(k) for k in range(40)]
        _same_files(stored, want, "file")
        heads = [ops.jpeg_parse_header(f, "any") for f in stored]
        assert ops.jpeg_decode_groups(heads) == [(0, 16), (16, 32), (32, 40)]
        try:
            import PIL  # noqa: F401
        except ImportError:
            PIL = None
        if PIL is not None:
            with VideoMJPEG(paths[False]) as plain:
                for k in range(40):
                    assert np.array_equal(video.get_frame(k), plain.get_frame(k)), k
    with VideoMJPEG(paths[True], {"decoder": "device"}) as video, VideoMJPEG(paths[False], {"decoder": "device"}) as plain:
        assert video.frame_count == 40
        for k in range(40):
            assert np.array_equal(video.get_frame(k), plain.get_frame(k)), k
