"""CPU: the optimised Huffman tables of DESIGN.md §9, "Optimised Huffman tables", and their host layer.

The restatement (tests/jpeg_optimize_checks.py) against the fixture tests/golden/mjpeg_optimized_v1.npz: libjpeg's own
tables for the counts of 61 files Pillow wrote with optimize=True, the chosen counts, and the small calls; Kraft sum
and cost of every chosen table against an independent heapq tree; Pillow's decode of the optimised streams against
its decode of the plain ones; va_jpeg_math.h compiled into a stand-alone program under sanitizers; optimize= through
ops.jpeg_encode, the writer, write_video and the composer with the encoder replaced by the restatement; the C ABI's
declarations and refusals."""
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_checks as J
import jpeg_decode_checks as D
import jpeg_optimize_checks as O
import jpeg_sampled_encode_checks as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLING = dict(O.LAYOUTS)


@pytest.fixture(scope="module")
def fx():
    return O.fixture(os.path.join(ROOT, "tests", "golden", "mjpeg_optimized_v1.npz"))[0]


def _table(freq):
    return O.table_bytes(*O.gen_optimal_table(freq))


# ------------------------------------------------------------------------------------------------ the definition
def test_restatement_builds_libjpeg_s_tables(fx):
    """every table of every file Pillow wrote, from the counts recovered from that file"""
    assert len(fx["pin"]) == 61 and sum(len(t) for _, _, t in fx["pin"]) == 240
    assert "200x312_q100_444" not in [name for name, _, _ in fx["pin"]]
    for name, counts, tables in fx["pin"]:
        assert len(counts) == len(tables) == (2 if name.endswith("mono") else 4)
        for k in range(len(counts)):
            assert np.array_equal(_table(counts[k]), tables[k]), (name, k)
    # the limit to 16 bits ran in some of them: their HUFFVAL is not in the order of the final lengths
    z = np.load(os.path.join(ROOT, "tests", "golden", "mjpeg_optimized_v1.npz"))
    assert len(z["pin_tables_odd"]) > 0


def test_chosen_counts_kraft_sum_and_cost(fx):
    names = [name for name, _, _ in fx["chosen"]]
    assert names[:7] == ["one_symbol", "two_symbols", "equal_256", "ones_256", "dc_shape", "fibonacci_40", "powers_40"]
    assert len(names) == 207 and names[7] == "random_000" and names[-1] == "random_199"
    deep = 0
    for name, freq, table in fx["chosen"]:
        assert np.array_equal(_table(freq), table), name
        bits, nsym = [int(v) for v in table[:16]], int(table[:16].sum())
        vals = [int(v) for v in table[16:16 + nsym]]
        assert sorted(vals) == [int(i) for i in np.flatnonzero(freq)] and not table[16 + nsym:].any(), name
        if nsym == 0:
            assert not freq.any(), name
            continue
        codes = J.huffman_codes(bits, vals)
        lengths = {sym: n for sym, (_, n) in codes.items()}
        assert max(lengths.values()) <= 16, name
        assert sum(2 ** (16 - n) for n in lengths.values()) < 2 ** 16, name                   # the Kraft sum is below 1
        assert all(code != (1 << n) - 1 for code, n in codes.values()), name                  # no code is all 1-bits
        # the code is complete with the reserved symbol in it: what the Kraft sum lacks is that symbol's code
        lack = 2 ** 16 - sum(2 ** (16 - n) for n in lengths.values())
        reserved = 16 - (lack.bit_length() - 1)
        assert lack == 2 ** (16 - reserved) and reserved >= max(lengths.values()), name
        cost = sum(int(freq[sym]) * n for sym, n in lengths.items()) + reserved
        best, depth = O.heap_cost(freq)
        if depth <= 16:
            assert cost == best, (name, cost, best)
        else:
            assert cost >= best, (name, cost, best)
            deep += 1
    by_name = {name: (freq, table) for name, freq, table in fx["chosen"]}
    assert [int(v) for v in by_name["one_symbol"][1][:17]] == [1] + [0] * 15 + [5]
    assert [int(v) for v in by_name["two_symbols"][1][:18]] == [1, 1] + [0] * 14 + [3, 200]
    assert O.heap_cost(by_name["fibonacci_40"][0])[1] > 16 and O.heap_cost(by_name["powers_40"][0])[1] > 32
    assert deep >= 2


def test_small_calls_equal_the_stored_streams_and_are_never_larger(fx):
    assert len(fx["calls"]) == 20 and {c[1] for c in fx["calls"]} == {"mono", "444", "422", "420"}
    for name, layout, quality, frames, files, tables, _ in fx["calls"]:
        got, got_tables = O.encode(frames, quality, SAMPLING[layout])
        assert got == files and np.array_equal(got_tables, tables), name
        plain = O._plain(frames, quality, SAMPLING[layout])
        assert sum(map(len, files)) <= sum(map(len, plain)), name
        pre, post = O.split_header(plain[0][:len(J.header(*frames.shape[1:3], 1 if frames.ndim == 3 else 3, quality))])
        for f, p in zip(files, plain):
            assert f.startswith(pre) and p.startswith(pre) and f[-2:] == b"\xff\xd9", name
            head, plain_head = D.parse_header(f, "any"), D.parse_header(p, "any")
            assert f[:head["scan_begin"]].endswith(post) and head["scan_begin"] <= plain_head["scan_begin"], name
            assert D.header_key(head)[:4] == D.header_key(plain_head)[:4], name
            # the same coefficients, so the same counts, under the new tables
            assert np.array_equal(O.file_counts(f, head)[0], O.file_counts(p, plain_head)[0]), name
        assert np.array_equal(sum(O.file_counts(f)[0] for f in files), O.call_counts(frames, quality, SAMPLING[layout])), name
    # the tables of a call of three frames are those of the sum, not any single frame's
    name, layout, quality, frames, files, tables, _ = [c for c in fx["calls"] if c[0] == "420_3x17x33_q90"][0]
    for k in range(3):
        assert not np.array_equal(O.encode(frames[k:k + 1], quality, (2, 2))[1], tables)


def test_pillow_decodes_the_optimised_streams_to_the_plain_streams_pixels(fx):
    """the stored decode (what Pillow saw when the fixture was written) makes the check repeatable without Pillow"""
    try:
        from PIL import Image
    except ImportError:
        Image = None
    import jpeg_subsampled_checks as S
    for call in fx["calls"]:
        name, layout, quality, frames, files = call[:5]
        seen = O.pillow_pixels(call)
        assert seen.shape == frames.shape and seen.dtype == np.uint8 and np.abs(call[6]).max() <= 4, name
        plain = O._plain(frames, quality, SAMPLING[layout])
        for k, (f, p) in enumerate(zip(files, plain)):
            assert np.array_equal(S.ideal_decode(f), S.ideal_decode(p)), (name, k)
            if Image is not None:
                a, b = (np.asarray(Image.open(io.BytesIO(data))) for data in (f, p))
                assert np.array_equal(a, b) and np.array_equal(a, seen[k]), (name, k)


def test_a_string_of_more_than_64_bits_is_a_valid_stream():
    """the frame with one coefficient behind a run of 62 (jpeg_optimize_checks.long_run_stack): its optimised file
    holds the plain file's coefficients, and Pillow reads the same pixels from both"""
    stack = O.long_run_stack()
    files, tables = O.encode(stack, 90, None)
    assert O.long_run_bits(stack, 90, tables) == (16, 69)
    plain = J.encode_frame(stack[3], 90)
    assert len(files[3]) != len(plain)
    got, want = D.decode_coefficients(files[3]), D.decode_coefficients(plain)
    assert got[1] == want[1] == 0 and np.array_equal(got[0], want[0]) and got[0][0, 0, 0, 63] != 0
    try:
        from PIL import Image
    except ImportError:
        return
    a, b = (np.asarray(Image.open(io.BytesIO(data))) for data in (files[3], plain))
    assert np.array_equal(a, b)


def test_pillow_s_own_gain_is_stored(fx):
    assert sorted(fx["ratios"]) == sorted("%s/%s" % (a, b) for a in ("smooth", "noise") for b, _ in O.LAYOUTS)
    assert all(0.85 < opt / plain < 0.95 for plain, opt in fx["ratios"].values())


# ------------------------------------------------------------------------------------------------ the header on the host
def test_tables_and_streams_on_the_host_under_sanitizers(fx, tmp_path):
    """va_jpeg_math.h's table construction, symbol counting and run-time encoder tables in a stand-alone program built
    with -fsanitize=address,undefined: its tables for every count of the fixture, and its counts, tables and entropy
    segments for every small call, are the restatement's"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "llvm", "bin", "clang++")
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or (
        rocm_clang if os.path.exists(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler: neither g++, c++ or clang++ on the PATH nor %s" % rocm_clang
    exe = str(tmp_path / "jpeg_optimize_shim")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "video-analysis_amd", "csrc"),
                           os.path.join(ROOT, "tests", "jpeg_optimize_shim.cpp"), "-o", exe])
    counts = np.concatenate([c for _, c, _ in fx["pin"]] + [c[None] for _, c, _ in fx["chosen"]]).astype(np.int64)
    want = np.concatenate([t for _, _, t in fx["pin"]] + [t[None] for _, _, t in fx["chosen"]])
    out = subprocess.run([exe], input=struct.pack("<2i", 0, len(counts)) + counts.tobytes(), capture_output=True,
                         check=True).stdout
    assert np.array_equal(np.frombuffer(out, np.uint8).reshape(-1, O.TABLE_BYTES), want)
    for name, layout, quality, frames, files, tables, _ in fx["calls"]:
        hh, vv = SAMPLING[layout] or (1, 1)
        n, h, w = frames.shape[:3]
        qt = J.quant_tables(quality)
        text = (struct.pack("<7i", 1, n, h, w, 1 if frames.ndim == 3 else 3, hh, vv) + qt[0].astype(np.uint8).tobytes()
                + qt[1].astype(np.uint8).tobytes() + frames.tobytes())
        out = subprocess.run([exe], input=text, capture_output=True, check=True).stdout
        assert np.array_equal(np.frombuffer(out[:8192], np.int64).reshape(2, 2, 256),
                              O.call_counts(frames, quality, SAMPLING[layout])), name
        at = 8192 + 4 * O.TABLE_BYTES
        got = np.frombuffer(out[8192:at], np.uint8).reshape(4, O.TABLE_BYTES)
        assert np.array_equal(got[:len(tables)], tables) and not got[len(tables):].any(), name
        for f in files:
            head = D.parse_header(f, "any")
            segs, bit = D.split_segments(f, head["scan_begin"], head["nseg"])
            assert bit == 0 and len(segs) == head["nseg"]
            for begin, end in segs:
                size = struct.unpack("<i", out[at:at + 4])[0]
                assert out[at + 4:at + 4 + size] == f[begin:end], name
                at += 4 + size
        assert at + 4 == len(out) and 0 < struct.unpack("<i", out[at:])[0] <= 59, name
    # a coefficient behind a run of 62 under a ZRL code of 16 bits: 69 bits, more than one 64-bit string holds
    stack = O.long_run_stack()
    files, tables = O.encode(stack, 90, None)
    assert O.long_run_bits(stack, 90, tables) == (16, 69)
    qt = J.quant_tables(90)
    text = (struct.pack("<7i", 1, 4, 256, 256, 1, 1, 1) + qt[0].astype(np.uint8).tobytes()
            + qt[1].astype(np.uint8).tobytes() + stack.tobytes())
    out = subprocess.run([exe], input=text, capture_output=True, check=True).stdout
    at = 8192 + 4 * O.TABLE_BYTES
    assert np.array_equal(np.frombuffer(out[8192:at], np.uint8).reshape(4, O.TABLE_BYTES)[:2], tables)
    for f in files:
        head = D.parse_header(f, "any")
        for begin, end in D.split_segments(f, head["scan_begin"], head["nseg"])[0]:
            size = struct.unpack("<i", out[at:at + 4])[0]
            assert out[at + 4:at + 4 + size] == f[begin:end]
            at += 4 + size
    assert at + 4 == len(out) and struct.unpack("<i", out[at:])[0] == 69


# ------------------------------------------------------------------------------------------------ the host layer
@pytest.fixture
def restated_encoder(monkeypatch):
    """video.ops.jpeg_encode replaced by the restatements; the calls are logged as (frames, quality, sampling, optimize)"""
    from video import ops
    log = []

    def jpeg_encode(frames, quality=90, color=None, stream=None, ret_packed=False, sampling=(1, 1), optimize=False):
        frames = np.asarray(frames)
        log.append((len(frames), quality, sampling, optimize))
        layout = None if frames.ndim == 3 else tuple(sampling)
        files = O.encode(frames, quality, layout)[0] if optimize else O._plain(frames, quality, layout)
        return E.packed(files) if ret_packed else files
    monkeypatch.setattr(ops, "jpeg_encode", jpeg_encode)
    return log


def test_host_layer_refuses_a_wrong_optimize_before_any_library_call(monkeypatch, tmp_path):
    from video import _hip, ops
    from video.io import file as vfile
    from video.io.backend_mjpeg import VideoWriterMJPEG
    from video.io.memory import VideoMemory

    def no_library(*args, **kwargs):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_hip, "lib", no_library)
    monkeypatch.setattr(_hip, "load_library", no_library)
    color = np.zeros((2, 16, 16, 3), np.uint8)
    for bad in (1, 0, None, "yes", "True", 1.0, (True,), np.uint8(1)):
        with pytest.raises(TypeError, match="optimize"):
            ops.jpeg_encode(color, optimize=bad)
        with pytest.raises(TypeError, match="optimize"):
            VideoWriterMJPEG(tmp_path / "bad.avi", (16, 16), 25, optimize=bad)
        with pytest.raises(TypeError, match="optimize"):
            vfile.write_video(VideoMemory(color, fps=30), str(tmp_path / "bad.avi"), optimize=bad)
    assert not (tmp_path / "bad.avi").exists()
    with pytest.raises(ValueError, match="ret_tables"):
        ops.jpeg_encode(color, ret_tables=True)
    assert ops.jpeg_encode(color[:0], optimize=True) == [] and ops.jpeg_encode(color[:0], optimize=np.True_) == []
    for bad in (np.zeros((2, 255), np.int64), np.zeros(256, np.float64), np.zeros((1, 2, 256), np.int64)):
        with pytest.raises(ValueError, match="counts"):
            ops.jpeg_optimal_tables(bad)
    with pytest.raises(ValueError, match="counts"):
        ops.jpeg_optimal_tables(np.full(256, -1, np.int64))
    with pytest.raises(ValueError, match="sum"):                     # the device adds a row's counts in 64 bits
        ops.jpeg_optimal_tables(np.full((2, 256), 2 ** 56, np.int64))
    with pytest.raises(ValueError, match="sum"):
        ops.jpeg_optimal_tables(np.full(256, 2 ** 63, np.uint64))
    assert ops.jpeg_optimal_tables(np.zeros((0, 256), np.int64)).shape == (0, ops.JPEG_TABLE_BYTES)
    assert ops.JPEG_TABLE_BYTES == O.TABLE_BYTES
    for c, sampling in ((1, (1, 1)), (3, (1, 1)), (3, (2, 1)), (3, (2, 2))):
        head = ops.jpeg_header(37, 53, c, 90, sampling)
        assert ops.jpeg_header_pieces(head) == O.split_header(head)
        pre, post = ops.jpeg_header_pieces(head)
        assert len(pre) + len(post) + (c + 1) // 2 * (33 + 183) == len(head)


def _clip(n, h, w, seed=3):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, 30 + 20 * t, (h, w, 3)) for t in range(n)]).astype(np.uint8)


def test_writer_writes_runs_of_its_batch(restated_encoder, tmp_path):
    from video import ops
    from video.io.backend_mjpeg import VideoMJPEG, VideoWriterMJPEG
    clip = _clip(7, 18, 34)
    path = tmp_path / "clip.avi"
    with VideoWriterMJPEG(path, (34, 18), 12.5, quality=75, batch=3, sampling="4:2:0", optimize=True) as writer:
        assert writer.optimize is True
        for f in clip:
            writer.write_frame(f)
    assert restated_encoder == [(3, 75, (2, 2), True), (3, 75, (2, 2), True), (1, 75, (2, 2), True)]
    want = sum((O.encode(clip[a:a + 3], 75, (2, 2))[0] for a in (0, 3, 6)), [])
    J.parse_avi(path.read_bytes())
    with VideoMJPEG(path) as video:
        stored = [video.get_frame_bytes(k) for k in range(7)]
    assert stored == want
    assert ops.jpeg_decode_groups([ops.jpeg_parse_header(f, "any") for f in stored]) == [(0, 3), (3, 6), (6, 7)]
    with VideoWriterMJPEG(tmp_path / "plain.avi", (34, 18), 25, batch=3) as writer:
        assert writer.optimize is False
        writer.write_frames(clip[:2])
    assert restated_encoder[3:] == [(2, 90, (1, 1), False)]           # the default: the call as it was


def test_write_video_and_the_composer_pass_optimize_on(restated_encoder, tmp_path, monkeypatch):
    import composer_checks as K
    from video import ops
    from video.io import file as vfile
    from video.io.backend_mjpeg import VideoMJPEG
    from video.io.composer import VideoComposer
    from video.io.memory import VideoMemory
    clip = _clip(5, 10, 12)
    path = str(tmp_path / "w.avi")
    vfile.write_video(VideoMemory(clip, fps=30), path, quality=60, batch=2, optimize=True)
    assert restated_encoder == [(2, 60, (1, 1), True)] * 2 + [(1, 60, (1, 1), True)]
    with VideoMJPEG(path) as video:
        assert [video.get_frame_bytes(k) for k in range(5)] == sum(
            (O.encode(clip[a:a + 2], 60, (1, 1))[0] for a in (0, 2, 4)), [])
    del restated_encoder[:]
    monkeypatch.setattr(ops, "compose_layers", lambda frames, layers, color=None, keep=False, stream=None:
                        K.compose_layers(frames, layers, color=color))
    monkeypatch.setattr(ops, "draw", lambda frames, commands, keep=False, stream=None: K.draw(frames, commands))
    vc = VideoComposer(str(tmp_path / "c.avi"), (12, 10), 25, True, batch=4, quality=70, sampling="4:2:2", optimize=True)
    for f in clip:
        vc.set_frame(f)
        vc.add_rectangle((2, 2, 6, 5), "w")
    vc.close()
    assert vc.frames_written == 5 and vc.sink.optimize is True
    assert {c[1:] for c in restated_encoder} == {(70, (2, 1), True)} and sum(c[0] for c in restated_encoder) == 5


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_declarations_and_refusals():
    import ctypes as C
    from video import _hip
    text = open(os.path.join(ROOT, "include", "videoanalysis_hip.h")).read()
    assert "int va_jpeg_encode_optimized_u8(const uint8_t *frames_dev, int n, int h, int w, int c, int luma_h, int luma_v," in text
    assert "int va_jpeg_optimal_tables(const int64_t *freq_dev, int t, uint8_t *bits_vals_out_dev, void *stream);" in text
    res, args = _hip.SIGNATURES["va_jpeg_encode_optimized_u8"]
    sampled = _hip.SIGNATURES["va_jpeg_encode_sampled_u8"][1]
    assert res is C.c_int and len(args) == 19 and args[:10] == sampled[:10] and args[13:] == sampled[10:]
    assert args[10] is C.c_void_p and args[11] is C.c_int and args[12] is C.c_void_p
    assert _hip.SIGNATURES["va_jpeg_optimal_tables"] == (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p])
    L = _hip.load_library()
    fn = L.va_jpeg_encode_optimized_u8
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data
    names = ["frames", "n", "h", "w", "c", "luma_h", "luma_v", "qt", "pre", "pre_bytes", "post", "post_bytes", "tables",
             "sizes", "offsets", "totals", "out", "cap", "stream"]
    ok = [p, 1, 8, 8, 3, 2, 2, p, p, 300, p, 20, p, p, p, p, p, 64, None]

    def call(**change):
        a = list(ok)
        for k, v in change.items():
            a[names.index(k)] = v
        return fn(*a), L.va_last_error().decode()
    for change, word in ((dict(n=-1), "size"), (dict(h=0), "size"), (dict(w=0), "size"), (dict(cap=-1), "size"),
                         (dict(pre_bytes=0), "size"), (dict(post_bytes=0), "size"), (dict(pre_bytes=-5), "size"),
                         (dict(pre_bytes=2 ** 31 - 1, post_bytes=2 ** 31 - 1), "size"),
                         (dict(c=2), "channels"), (dict(c=4), "channels"),
                         (dict(frames=None), "NULL"), (dict(qt=None), "NULL"), (dict(pre=None), "NULL"),
                         (dict(post=None), "NULL"), (dict(tables=None), "NULL"),
                         (dict(sizes=None), "NULL"), (dict(offsets=None), "NULL"), (dict(totals=None), "NULL"),
                         (dict(out=None), "NULL"), (dict(sizes=p + 4), "aligned"), (dict(offsets=p + 2), "aligned"),
                         (dict(totals=p + 1), "aligned"), (dict(h=65536), "16-bit"), (dict(w=70000), "16-bit"),
                         (dict(luma_h=1, luma_v=2), "sampling"), (dict(luma_h=4, luma_v=1), "sampling"),
                         (dict(luma_h=0, luma_v=0), "sampling"), (dict(c=1), "3 channels")):
        rc, message = call(**change)
        assert rc == -22 and word in message and "va_jpeg_encode_optimized_u8" in message, (change, rc, message)
    # the order of the checks is the plain call's: sizes, channels, NULL, alignment, 16 bits, the sampling, its channels
    assert "size" in call(post_bytes=0, c=2)[1] and "channels" in call(c=2, post=None)[1]
    assert "NULL" in call(tables=None, sizes=p + 4)[1] and "aligned" in call(sizes=p + 4, h=65536)[1]
    assert "16-bit" in call(h=65536, luma_h=3)[1] and "sampling is" in call(luma_h=3, c=1)[1]
    assert call(n=0, frames=None, post=None, tables=None, luma_h=7)[0] == 0      # n = 0 is VA_OK, nothing is looked at
    tab = L.va_jpeg_optimal_tables
    for a, word in (((p, -1, p, None), "negative"), ((None, 1, p, None), "NULL"), ((p, 1, None, None), "NULL"),
                    ((p + 4, 1, p, None), "aligned")):
        assert tab(*a) == -22 and word in L.va_last_error().decode() and "va_jpeg_optimal_tables" in L.va_last_error().decode()
    assert tab(None, 0, None, None) == 0
    assert not buf.any()


def test_product_does_not_import_the_restatement():
    pkg = os.path.join(ROOT, "video-analysis_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                assert "jpeg_optimize_checks" not in open(os.path.join(dirpath, f)).read(), f
