"""CPU: the Motion-JPEG decoder's definitions ("Motion-JPEG decoding") and their host layer.

The restatement tests/jpeg_decode_checks.py against the fixture tests/golden/mjpeg_decode_v1.npz and against the ideal
decode within the IDCT bounds, the header parser of video.ops on the accepted and the refused streams, the grouping
of mixed headers, the segment splitter on hand-made bytes, the device's Huffman tables as the host builds them, the
C ABI's declaration and refusals, VideoMJPEG with its default decoder, and va_jpeg_decode_math.h compiled into a
stand-alone program under sanitizers (tests/jpeg_decode_shim.cpp, the one shim of every sampling layout), on this
fixture and on records of this and the subsampled fixture alternating in one run."""
import os

import numpy as np
import pytest

import jpeg_checks as J
import jpeg_decode_checks as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plus(pillow, difference):
    """the fixture stores the expected pixels as their int8 difference from Pillow's decode of the same stream"""
    return (pillow.astype(np.int16) + difference).astype(np.uint8)


@pytest.fixture(scope="module")
def golden():
    return (np.load(os.path.join(ROOT, "tests", "golden", "mjpeg_v1.npz"), allow_pickle=False),
            np.load(os.path.join(ROOT, "tests", "golden", "mjpeg_decode_v1.npz"), allow_pickle=False))


def _hostile_pixels(enc, dec, name):
    """(c) stores pixels as their difference modulo 256 from those of the intact stream the case was made from"""
    source = name.rsplit("_", 2)[0] if "_cut_" in name or "_rst_" in name or "_no_eoi" in name else name.rsplit("_", 1)[0]
    return _plus(enc["pillow_" + source], dec["a_dpx_" + source]) + dec["c_dpx_" + name]


@pytest.fixture(scope="module")
def cases(golden):
    """{'a' | 'b' | 'c': [(name, bytes, expected pixels, expected status)]}"""
    enc, dec = golden
    return {"a": [(str(n), enc["bytes_" + n].tobytes(), _plus(enc["pillow_" + n], dec["a_dpx_" + n]), 0)
                 for n in dec["names_a"]],
            "b": [(str(n), dec["b_bytes_" + n].tobytes(), _plus(dec["b_pillow_" + n.rsplit("_", 1)[0]], dec["b_dpx_" + n.rsplit("_", 1)[0]]), 0)
                  for n in dec["names_b"]],
            "c": [(str(n), dec["c_bytes_" + n].tobytes(), _hostile_pixels(enc, dec, n), int(s))
                  for n, s in zip(dec["names_c"], dec["status_c"])]}


# ------------------------------------------------------------------------------------------------ the definition
def test_restatement_still_decodes_to_the_fixture(cases):
    assert (len(cases["a"]), len(cases["b"]), len(cases["c"])) == (120, 96, 28)
    for kind in "abc":
        for name, data, want, want_status in cases[kind]:
            got, status = D.decode(data)
            assert status == want_status and got.dtype == np.uint8 and np.array_equal(got, want), name
    bits = 0
    for _, _, _, s in cases["c"]:
        bits |= s
    assert bits == D.BAD_CODE | D.OVERRUN | D.TRUNCATED | D.MARKER


def test_accuracy_condition(golden, cases):
    """component samples within 1 of the float64 IDCT of the same coefficients, pixels within 1 (monochrome) and
    R 3, G 3, B 4 (colour) of the ideal decode, the clamp never active; Pillow's decode of (b), recorded when the
    fixture was written, within the same bounds of the ideal decode"""
    enc, dec = golden
    for name, data, want, _ in cases["a"] + cases["b"]:
        head = D.parse_header(data)
        coefs, status = D.decode_coefficients(data, head)
        f, clamped = D.dequantised(coefs, head["qtables"])
        assert status == 0 and not clamped, name
        assert np.abs(D.integer_planes(f) - D.float_planes(f)).max() <= 1, name
        ideal = D.ideal_decode(data, head)
        bound = 1 if want.ndim == 2 else np.array([3, 3, 4])
        assert (np.abs(want.astype(int) - ideal.astype(int)) <= bound).all(), name
    for name, data, _, _ in cases["a"]:
        assert np.array_equal(D.ideal_decode(data), J.ideal_decode(data)), name
    for base in dec["bases_b"]:
        ideal = D.ideal_decode(dec["b_bytes_%s_plain" % base].tobytes())
        bound = 1 if ideal.ndim == 2 else np.array([3, 3, 4])
        assert (np.abs(dec["b_pillow_" + base].astype(int) - ideal.astype(int)) <= bound).all(), base
    assert dec["worst_component"] <= 1 and dec["worst_mono"] <= 1 and (dec["worst_rgb"] <= (3, 3, 4)).all()


def test_int32_bound_of_the_inverse_transform():
    """the bound DESIGN.md carries: every intermediate fits int32 for any clamped input"""
    t, _ = J.dct_matrix()
    col = int(np.abs(t).sum(axis=0).max())
    assert col == 21641
    first = 2048 * col + (1 << (D.SHIFT1 - 1))
    kept = first >> D.SHIFT1
    second = kept * col + (1 << (D.SHIFT2 - 1))
    assert first < 2 ** 31 and second < 2 ** 31
    worst = np.where(t >= 0, 2047, -2048)                       # the signs of a row of T: the largest sums
    f = np.stack([np.outer(worst[:, y], worst[:, n]) for y in range(8) for n in range(8)]).reshape(1, 8, 8, 8, 8)
    assert D.integer_planes(np.clip(f, -2048, 2047)).max() <= 255


# ------------------------------------------------------------------------------------------------ the parser
def test_header_parser_on_accepted_streams(cases):
    from video import ops
    for name, data, want, _ in cases["a"] + cases["b"] + cases["c"]:
        head, mine = D.parse_header(data), ops.jpeg_parse_header(data)
        assert D.header_key(head) == D.header_key(mine) and head["scan_begin"] == mine["scan_begin"], name
        assert (mine["h"], mine["w"]) == want.shape[:2] and mine["c"] == (3 if want.ndim == 3 else 1), name
        assert mine["nseg"] == head["nseg"] == -(-(-(-mine["h"] // 8) * -(-mine["w"] // 8)) // mine["ri"])
        assert mine["qtables"].shape == (mine["c"], 64) and mine["qtables"].dtype == np.uint8
    by_name = {c[0]: ops.jpeg_parse_header(c[1]) for c in cases["b"]}
    assert (by_name["RGB_q85_37x53_plain"]["ri"], by_name["RGB_q85_37x53_plain"]["nseg"]) == (35, 1)
    assert (by_name["RGB_q85_37x53_rows"]["ri"], by_name["RGB_q85_37x53_rows"]["nseg"]) == (7, 5)
    assert (by_name["RGB_q85_37x53_blocks3"]["ri"], by_name["RGB_q85_37x53_blocks3"]["nseg"]) == (3, 12)
    assert by_name["RGB_q85_37x53_optimized"]["huff"] != by_name["RGB_q85_37x53_plain"]["huff"]
    annex_k = tuple((ops.JPEG_DHT[t], ops.JPEG_DHT[0x10 | t]) for t in (0, 1, 1))
    assert tuple(ops.jpeg_parse_header(cases["a"][0][1])["huff"]) == annex_k[:1]


def test_header_parser_refuses(golden, cases):
    from video import ops
    _, dec = golden
    assert list(dec["names_d"]) == ["pillow_420", "pillow_progressive", "sof_12bit", "two_scans"]
    for name, word in zip(dec["names_d"], dec["words_d"]):
        data = dec["d_bytes_" + name].tobytes()
        for parse in (ops.jpeg_parse_header, D.parse_header):
            with pytest.raises(ValueError) as err:
                parse(data)
            assert str(word) in str(err.value), (name, err.value)
    good = cases["a"][-1][1]
    sof, dqt = good.index(b"\xff\xc0"), good.index(b"\xff\xdb")
    for change, word in (((sof + 1, 0xC1), "extended"), ((sof + 1, 0xC9), "arithmetic"), ((sof + 1, 0xC3), "lossless"),
                         ((dqt + 4, 0x10), "16-bit"), ((0, 0x00), "SOI"), ((sof + 9, 2), "components")):
        bad = bytearray(good)
        bad[change[0]] = change[1]
        with pytest.raises(ValueError) as err:
            ops.jpeg_parse_header(bytes(bad))
        assert word in str(err.value), (change, err.value)
    with pytest.raises(ValueError):
        ops.jpeg_parse_header(good[:100])
    dnl = good[:sof] + b"\xff\xdc\x00\x04\x00\x08" + good[sof:]
    with pytest.raises(ValueError) as err:
        ops.jpeg_parse_header(dnl)
    assert "DNL" in str(err.value)


def test_refusals_agree_with_what_pillow_reads_from_the_headers(golden, cases):
    """an independent reading of the same headers (Pillow's own JPEG parser: sample bits, layers with their sampling
    factors, the progressive flag): ops.jpeg_parse_header takes a file exactly when Pillow reports 8 bits, not
    progressive, and 1 layer or 3 layers that are all 1 x 1, with Pillow's size and layer count.  (What Pillow's
    header parse does not show -- the number of scans -- is covered by the fixture's two_scans case alone.)"""
    Image = pytest.importorskip("PIL.Image")
    import io
    from video import ops
    _, dec = golden
    rng = np.random.default_rng(5)
    rgb, grey = rng.integers(0, 256, (16, 24, 3), dtype=np.uint8), rng.integers(0, 256, (16, 24), dtype=np.uint8)

    def written(frame, **kw):
        buf = io.BytesIO()
        Image.fromarray(frame).save(buf, "JPEG", quality=75, **kw)
        return buf.getvalue()
    files = [c[1] for c in cases["b"][::7]] + [c[1] for c in cases["a"][::11]]
    files += [dec["d_bytes_" + n].tobytes() for n in ("pillow_420", "pillow_progressive", "sof_12bit")]
    files += [written(rgb, subsampling=s) for s in (0, 1, 2)] + [written(rgb, subsampling=0, progressive=True)]
    files += [written(grey), written(grey, progressive=True), written(rgb, subsampling=0, optimize=True)]
    taken = refused = 0
    for data in files:
        try:
            image = Image.open(io.BytesIO(data))
            sampling = [(h, v) for _, h, v, _ in image.layer]
            fits = (image.bits == 8 and not image.info.get("progressive") and image.layers in (1, 3)
                    and (image.layers == 1 or all(hv == (1, 1) for hv in sampling)))
        except Exception:
            image, fits = None, False                      # Pillow does not read the file at all (12-bit SOF0)
        if fits:
            head = ops.jpeg_parse_header(data)
            assert (head["w"], head["h"]) == image.size and head["c"] == image.layers
            taken += 1
        else:
            with pytest.raises(ValueError):
                ops.jpeg_parse_header(data)
            refused += 1
    assert taken >= 20 and refused >= 7


def test_grouping_of_mixed_headers(cases):
    from video import ops
    by_name = {c[0]: c[1] for c in cases["a"] + cases["b"]}
    order = ["noise_q90_37x53x3", "flat_37x53x3", "noise_q50_37x53x3", "RGB_q85_37x53_plain", "RGB_q85_37x53_rows",
             "RGB_q85_37x53_rows", "zeros_37x53x3", "full_37x53x3"]
    heads = [ops.jpeg_parse_header(by_name[n]) for n in order]
    assert ops.jpeg_decode_groups(heads) == [(0, 2), (2, 3), (3, 4), (4, 6), (6, 8)]
    assert ops.jpeg_decode_groups([]) == [] and ops.jpeg_decode_groups(heads[:1]) == [(0, 1)]


# ------------------------------------------------------------------------------------------------ the splitter
def test_segment_splitter_on_hand_made_bytes():
    rst = lambda k: bytes([0xFF, 0xD0 + k])
    eoi = b"\xff\xd9"
    # FF FF D0: the first FF is a byte of the segment, the marker is the second FF
    assert D.split_segments(b"\x12\xff\xff\xd0\x34" + eoi, 0, 2) == ([(0, 2), (4, 5)], 0)
    # a marker as the last two bytes, and a file that ends without one
    assert D.split_segments(b"\x01\x02" + eoi, 0, 1) == ([(0, 2)], 0)
    assert D.split_segments(b"\x01\x02", 0, 1) == ([(0, 2)], D.MARKER)
    assert D.split_segments(b"\x01\x02\xff", 0, 1) == ([(0, 3)], D.MARKER)            # cut behind an FF
    # an empty segment
    assert D.split_segments(b"\x01" + rst(0) + rst(1) + b"\x02" + eoi, 0, 3) == ([(0, 1), (3, 3), (5, 6)], 0)
    # stuffing is no marker; scan_begin is where the search starts
    assert D.split_segments(eoi + b"\xff\x00\x05" + eoi, 2, 1) == ([(2, 5)], 0)
    # a wrong RST ends the scan; the later segments are missing
    assert D.split_segments(b"\x01" + rst(1) + b"\x02" + eoi, 0, 2) == ([(0, 1), None], D.MARKER)
    # more or fewer segments than expected
    assert D.split_segments(b"\x01" + rst(0) + b"\x02" + eoi, 0, 1) == ([(0, 1)], D.MARKER)
    assert D.split_segments(b"\x01" + eoi, 0, 2) == ([(0, 1), None], D.MARKER)
    # RST numbers wrap after 8
    body = b"".join(b"\x07" + rst(k % 8) for k in range(9)) + b"\x07" + eoi
    segs, bit = D.split_segments(body, 0, 10)
    assert bit == 0 and segs == [(3 * k, 3 * k + 1) for k in range(10)]
    assert D.unstuffed(b"\xff\x00\xff\x00\x00\xff", 0, 6) == b"\xff\xff\x00\xff"
    assert D.unstuffed(b"\xff\x00", 0, 1) == b"\xff"


def test_device_tables_decode_every_code(cases):
    """the look-ahead and the long-code arrays of ops._jpeg_decode_table, walked as huff_step walks them, give back
    every code of Annex K and of a Pillow-optimised table"""
    from video import ops
    tables = [ops.JPEG_DHT[k] for k in sorted(ops.JPEG_DHT)]
    optimised = ops.jpeg_parse_header({c[0]: c[1] for c in cases["b"]}["RGB_q85_37x53_optimized"])["huff"]
    tables += [t for pair in optimised for t in pair]
    for bits, vals in tables:
        raw = ops._jpeg_decode_table(bits, vals)
        assert len(raw) == ops.JPEG_HUFF_DECODE_BYTES == 1416
        look = np.frombuffer(raw[:1024], np.uint16)
        maxcode, valoff = np.frombuffer(raw[1024:1092], np.int32), np.frombuffer(raw[1092:1160], np.int32)
        symbols = np.frombuffer(raw[1160:], np.uint8)
        for sym, (code, length) in J.huffman_codes(list(bits), list(vals)).items():
            for tail in (0, (1 << (16 - length)) - 1):
                peek = (code << (16 - length)) | tail
                e = int(look[peek >> 7])
                if e:
                    assert (e >> 8, e & 255) == (length, sym)
                    continue
                found = [l for l in range(10, 17) if (peek >> (16 - l)) <= maxcode[l]][0]
                assert found == length and symbols[(valoff[found] + (peek >> (16 - found))) & 255] == sym
        if sum(bits) < 256 and list(bits) == list(ops.JPEG_DHT[0x10][0]):
            assert look[511] == 0 and all((0xFFFF >> (16 - l)) > maxcode[l] for l in range(10, 17))    # no code of 1s


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_declaration_and_refusals():
    import ctypes as C
    from video import _hip
    text = open(os.path.join(ROOT, "include", "videoanalysis_hip.h")).read()
    assert "VideoOpenCV.get_frame" in text and "video/io/file.py:37-46" in text and "backend_opencv.py" in text
    for name, value in (("BAD_CODE", D.BAD_CODE), ("OVERRUN", D.OVERRUN), ("TRUNCATED", D.TRUNCATED),
                        ("MARKER", D.MARKER)):
        assert "#define VA_JPEG_STATUS_%s %d " % (name, value) in text
    res, args = _hip.SIGNATURES["va_jpeg_decode_u8"]
    assert res is C.c_int and len(args) == 16 and args[14] is C.c_int64
    assert _hip.SIGNATURES["va_jpeg_decode_workspace_bytes"] == (C.c_size_t, [C.c_int] * 5)
    L = _hip.load_library()
    fn = L.va_jpeg_decode_u8
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data
    names = ["bytes", "offsets", "scan", "n", "h", "w", "c", "ri", "qt", "huff", "huff_bytes", "out", "status", "ws",
             "ws_bytes", "stream"]
    ok = [p, p, p, 1, 8, 8, 1, 1, p, p, 2 * 1416, p, p, p, 1 << 20, None]

    def call(**change):
        a = list(ok)
        for k, v in change.items():
            a[names.index(k)] = v
        return fn(*a), L.va_last_error().decode()
    for change, word in ((dict(n=-1), "size"), (dict(h=0), "size"), (dict(w=0), "size"), (dict(ri=0), "size"),
                         (dict(ws_bytes=-1), "size"), (dict(c=2), "channels"), (dict(c=4), "channels"),
                         (dict(bytes=None), "NULL"), (dict(offsets=None), "NULL"), (dict(scan=None), "NULL"),
                         (dict(qt=None), "NULL"), (dict(huff=None), "NULL"), (dict(out=None), "NULL"),
                         (dict(status=None), "NULL"), (dict(ws=None), "NULL"), (dict(offsets=p + 4), "aligned"),
                         (dict(scan=p + 2), "aligned"), (dict(huff=p + 1), "aligned"), (dict(status=p + 2), "aligned"),
                         (dict(ws=p + 8), "aligned"), (dict(h=65536), "16-bit"), (dict(w=70000), "16-bit"),
                         (dict(huff_bytes=1416), "tables"), (dict(c=3), "tables")):
        rc, message = call(**change)
        assert rc == -22 and word in message, (change, rc, message)
    # the order of the checks: sizes, channels, NULL, alignment, 16 bits, tables, then the workspace (VA_ERR_RANGE)
    assert "size" in call(h=0, c=2)[1] and "channels" in call(c=2, bytes=None)[1]
    assert "NULL" in call(bytes=None, offsets=p + 4)[1] and "aligned" in call(offsets=p + 4, h=65536)[1]
    assert "16-bit" in call(h=65536, huff_bytes=7)[1] and "tables" in call(huff_bytes=7, ws_bytes=0)[1]
    rc, message = call(ws_bytes=100)
    assert rc == -34 and "one frame" in message
    assert call(n=0, bytes=None, c=3, ws=None)[0] == 0                       # n = 0 is VA_OK, nothing is looked at
    assert not buf.any()
    size = L.va_jpeg_decode_workspace_bytes
    assert size(1, 8, 8, 1, 1) == 256 + 256 and size(0, 8, 8, 1, 1) == 0 and size(1, 8, 8, 2, 1) == 0
    assert size(32, 1080, 1920, 3, 240) >= 32 * (3 * 135 * 240 * 128 + 135 * 16)
    assert size(32, 1080, 1920, 3, 240) < 32 * (3 * 135 * 240 * 128 + 135 * 16) + 1024


# ------------------------------------------------------------------------------------------------ VideoMJPEG
def test_default_decoder_is_unchanged(tmp_path, monkeypatch):
    """without parameters get_frame takes the Pillow path as before and never calls ops.jpeg_decode; get_frames
    makes one ops.jpeg_decode call for its range"""
    from video import ops
    from video.io.backend_mjpeg import VideoMJPEG, VideoWriterMJPEG
    from video.io.file import load_any_video
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (5, 9, 17), dtype=np.uint8)

    def restated_encode(stack, quality=90, color=None, stream=None, ret_packed=False):
        files = J.encode(np.asarray(stack), quality)
        offsets = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)
        return (np.frombuffer(b"".join(files), np.uint8), offsets) if ret_packed else files
    calls = []

    def restated_decode(streams, color=None, stream=None, keep=False, ret_status=False):
        calls.append((len(streams), color, keep))
        return np.stack([D.decode(s)[0] for s in streams])
    monkeypatch.setattr(ops, "jpeg_encode", restated_encode)
    monkeypatch.setattr(ops, "jpeg_decode", restated_decode)
    path = str(tmp_path / "clip.avi")
    with VideoWriterMJPEG(path, size=(17, 9), fps=25, is_color=False, quality=90) as writer:
        for f in frames:
            writer.write_frame(f)
    want = np.stack([D.decode(J.encode_frame(f, 90))[0] for f in frames])
    for video in (VideoMJPEG(path), load_any_video(path), VideoMJPEG(path, {"decoder": "pillow"})):
        with video:
            assert video._decoder == "pillow"
            try:
                import PIL  # noqa: F401
            except ImportError:
                with pytest.raises(ImportError):
                    video.get_frame(0)
            else:
                got = np.stack([f for f in video])
                assert got.shape == want.shape and np.abs(got.astype(int) - want).max() <= 2
                assert np.array_equal(video.get_frame(-1), video[4])
            assert calls == []
    with load_any_video(path, {"decoder": "device"}) as video:
        assert np.array_equal(np.stack([f for f in video]), want) and calls == [(5, False, False)]
        assert np.array_equal(video[-2], want[3]) and len(calls) == 1
        assert np.array_equal(video.get_frames(1, 4), want[1:4]) and calls[-1] == (3, False, False)
        video.get_device_frames(2, None)
        assert calls[-1] == (3, False, True)
    with pytest.raises(ValueError):
        VideoMJPEG(path, {"decoder": "opencv"})


def test_run_frames_refuses_before_it_touches_the_device():
    from video.engine import FrameEngine

    class Frames(object):
        n, shape, buf = 2, (2, 5, 5), None
    engine = FrameEngine.__new__(FrameEngine)
    engine.dtype, engine.prepare, engine.height, engine.width, engine.channels = np.dtype(np.uint8), None, 4, 4, 1
    engine.max_batch = 8
    with pytest.raises(ValueError):
        engine.run_frames(Frames())
    engine.dtype = np.dtype(np.float32)
    with pytest.raises(TypeError):
        engine.run_frames(Frames())


# ------------------------------------------------------------------------------------------------ the header
def _with_cuts(everything, sources, decode):
    """`everything` and, hand-made from each of `sources`: a file that is its header alone, and one that ends with FF.
    [(name, bytes, expected pixels, expected status, the header to decode under)]"""
    from video import ops
    out = [(name, data, want, status, ops.jpeg_parse_header(data, sampling="any")) for name, data, want, status in everything]
    for name, data, _, _ in sources:
        head = ops.jpeg_parse_header(data, sampling="any")
        for cut in (data[:head["scan_begin"]], data[:head["scan_begin"] + 1] + b"\xff"):
            pixels, status = decode(cut, D.parse_header(data, sampling="any"))
            assert status & D.MARKER
            out.append((name + " cut", cut, pixels, status, head))
    return out


def _check_shim(exe, everything):
    from video import ops
    lines = D.run_shim(exe, [D.shim_record(data, head, ops._jpeg_decode_table) for _, data, _, _, head in everything])
    assert len(lines) == len(everything)
    for (name, _, want, want_status, _), line in zip(everything, lines):
        assert line == D.shim_line(want, want_status), name


def test_decode_math_header_on_the_host_under_sanitizers(cases, tmp_path):
    """va_jpeg_decode_math.h compiled for the host with -fsanitize=address,undefined into a stand-alone program that
    decodes every fixture stream, the hostile ones included, from a heap buffer of exactly the stream's size; its
    status words and the hash of its pixels are the restatement's"""
    everything = _with_cuts(cases["a"] + cases["b"] + cases["c"], (cases["a"][5], cases["a"][-1]), D.decode)
    assert len(everything) == 120 + 96 + 28 + 4
    _check_shim(D.build_shim(ROOT, tmp_path), everything)


def test_layouts_interleaved_in_one_run_of_the_host_program(cases, tmp_path):
    """records of this fixture and of the subsampled one, alternating, in a single run of the same program: no state
    of one layout leaks into the next record"""
    import jpeg_subsampled_checks as S
    sub = S.fixture_cases(os.path.join(ROOT, "tests", "golden", "mjpeg_subsampled_v1.npz"))[0]
    plain = _with_cuts((cases["a"] + cases["b"])[::9] + cases["c"], cases["a"][5:6], D.decode)
    sampled = _with_cuts(sub["a"][::8] + sub["b"], [c for c in sub["a"] if c[0] == "420_q85_17x33_rows"], S.decode)
    mixed = [x for pair in zip(plain, sampled) for x in pair]
    layouts = [(x[4]["c"],) + tuple(x[4]["sampling"]) for x in mixed]
    assert set(layouts) == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)} and len(mixed) >= 100
    assert all(a != b for a, b in zip(layouts, layouts[1:]))
    _check_shim(D.build_shim(ROOT, tmp_path), mixed)


def test_product_does_not_import_the_restatement():
    pkg = os.path.join(ROOT, "video-analysis_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                assert "jpeg_decode_checks" not in open(os.path.join(dirpath, f)).read(), f
