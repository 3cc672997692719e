"""CPU: the Motion-JPEG definitions ("Motion-JPEG") and their host layer.

The restatement tests/jpeg_checks.py against the fixture tests/golden/mjpeg_v1.npz (its bytes, which Pillow decoded
within the IDCT bounds when the fixture was written), the tables against a Pillow-written file where Pillow exists,
the header, the stuffing and padding rules, the AVI writer and reader with ops.jpeg_encode replaced by the
restatement, write_video, the composer with a file name and with a write_frames sink, the C ABI's declaration and
refusals, and va_jpeg_math.h compiled into a stand-alone program under sanitizers."""
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_checks as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "mjpeg_v1.npz"), allow_pickle=False)


@pytest.fixture
def restated_encoder(monkeypatch):
    """video.ops.jpeg_encode replaced by the restatement; the calls are logged as (type, frames, quality)"""
    from video import ops
    log = []

    def jpeg_encode(frames, quality=90, color=None, stream=None, ret_packed=False):
        frames = np.asarray(frames)
        log.append((len(frames), quality, color))
        files = J.encode(frames, quality)
        if not ret_packed:
            return files
        offsets = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)
        return np.frombuffer(b"".join(files), np.uint8), offsets
    monkeypatch.setattr(ops, "jpeg_encode", jpeg_encode)
    return log


# ------------------------------------------------------------------------------------------------ the definition
def test_restatement_still_writes_the_fixture_s_bytes(fixture):
    names = list(fixture["names"])
    assert len(names) == 120
    for name in names:
        got = J.encode_frame(fixture["frame_" + name], int(fixture["quality_" + name]))
        assert got == fixture["bytes_" + name].tobytes(), name
    stuffed = sum(fixture["bytes_" + n].tobytes().count(b"\xff\x00") for n in names if n.startswith("noise"))
    assert stuffed > 100


def test_fixture_streams_decode_to_what_pillow_saw(fixture):
    """the ideal decode of a sample of the streams is within the recorded bounds of Pillow's decode"""
    assert fixture["pillow_worst_mono"].tolist() <= [1] and (fixture["pillow_worst_rgb"] <= [3, 3, 4]).all()
    differ, total = fixture["quantised_differ"]
    assert 0 < differ < total // 100
    for name in ("noise_q90_9x17x1", "noise_q100_9x17x3", "checker_8x8x3", "lastzigzag_37x53x1", "zeros_1x1x3"):
        ideal = J.ideal_decode(fixture["bytes_" + name].tobytes())
        seen = fixture["pillow_" + name]
        assert ideal.shape == seen.shape == fixture["frame_" + name].shape
        err = np.abs(ideal.astype(int) - seen.astype(int)).reshape(-1, 3 if ideal.ndim == 3 else 1).max(axis=0)
        assert (err <= ([3, 3, 4] if ideal.ndim == 3 else [1])).all(), (name, err)


def test_integer_transform_is_within_one_of_the_float_transform(fixture):
    for name in ("noise_q100_37x53x3", "noise_q1_37x53x1", "checker_37x53x1", "noise_q50_80x16x3"):
        tables = J.quant_tables(int(fixture["quality_" + name]))
        for i, plane in enumerate(J.planes_of(fixture["frame_" + name])):
            d = J.forward(plane, tables[min(i, 1)]) - J.float_quantised(plane, tables[min(i, 1)])
            assert np.abs(d).max() <= 1


def test_extreme_categories_and_runs_are_in_the_fixture(fixture):
    """all 0 / all 255: the largest DC difference; the checkerboards at quality 100: the largest AC and DC sizes; the
    last-zigzag blocks: three ZRLs and run 14; a flat frame: EOB only"""
    _, _, coefs, _ = J.decode_coefficients(fixture["bytes_zeros_8x8x1"].tobytes())
    assert coefs[0][0, 0, 0] == -1024 // J.quant_tables(90)[0][0] or coefs[0][0, 0, 0] < -300
    _, _, coefs, _ = J.decode_coefficients(fixture["bytes_blockchecker_80x16x1"].tobytes())
    assert coefs[0][:, :, 0].min() == -1024 and coefs[0][:, :, 0].max() >= 1016       # DC differences of size 11
    _, _, coefs, _ = J.decode_coefficients(fixture["bytes_checker_8x8x1"].tobytes())
    assert np.abs(coefs[0][0, 0, 1:]).max() >= 512                                    # an AC coefficient of size 10
    _, _, coefs, _ = J.decode_coefficients(fixture["bytes_lastzigzag_37x53x1"].tobytes())
    inner = coefs[0][:4, :6]
    assert (inner[:, :, 63] != 0).all() and (inner[:, :, 1:63] == 0).all()
    _, _, coefs, _ = J.decode_coefficients(fixture["bytes_flat_37x53x3"].tobytes())
    assert all((c[:, :, 1:] == 0).all() for c in coefs)


def test_tables_against_a_pillow_file():
    Image = pytest.importorskip("PIL.Image")
    from video import ops
    rng = np.random.default_rng(0)
    frame = rng.integers(0, 256, (16, 16, 3), dtype=np.uint8)
    for quality in (1, 10, 25, 49, 50, 51, 75, 90, 95, 100):
        buf = io.BytesIO()
        Image.fromarray(frame).save(buf, "JPEG", quality=quality, subsampling=0, optimize=False)
        segs, _, _ = J.parse(buf.getvalue())
        written = {p[0]: np.array(list(p[1:65])) for m, p in segs if m == 0xDB}          # zigzag order, as in the file
        for t, (mine, theirs) in enumerate(zip(J.quant_tables(quality), ops.jpeg_tables(quality))):
            assert np.array_equal(mine[J.ZIGZAG], written[t]), (quality, t)
            assert np.array_equal(mine, theirs) and theirs.dtype == np.uint8
        # Image.quantization: natural order in this Pillow, zigzag in older ones -- one of the two
        reported = Image.open(io.BytesIO(buf.getvalue())).quantization
        for t, mine in enumerate(J.quant_tables(quality)):
            assert list(reported[t]) in (mine.tolist(), mine[J.ZIGZAG].tolist()), (quality, t)
    payloads = []
    for m, p in segs:
        if m == 0xC4:
            while p:
                n = 17 + sum(p[1:17])
                payloads.append(bytes(p[:n]))
                p = p[n:]
    assert sorted(payloads) == sorted(J.dht_payload(k) for k in J.DHT)
    for key, (bits, vals) in ops.JPEG_DHT.items():
        assert bytes((key,) + bits + vals) == J.dht_payload(key)


def test_tables_and_quality_rule():
    from video import ops
    assert J.quant_tables(50)[0].tolist() == J.BASE_LUMA.tolist() and J.quant_tables(50)[1].tolist() == J.BASE_CHROMA.tolist()
    assert set(J.quant_tables(100)[0]) == {1} and J.quant_tables(1)[0].max() == 255
    assert J.quant_tables(25)[0][0] == (16 * 200 + 50) // 100
    for bad in (0, 101, 50.5, True):
        with pytest.raises(ValueError):
            ops.jpeg_tables(bad)
    t, a = J.dct_matrix()
    assert np.allclose(a @ a.T, np.eye(8)) and t[0].tolist() == [2896] * 8 and t[1, 0] == 4017


def test_header_fields_and_lengths():
    from video import ops
    for h, w, c, q in ((1, 1, 1, 90), (37, 53, 3, 50), (1080, 1920, 3, 90), (65535, 65535, 1, 1)):
        head = ops.jpeg_header(h, w, c, q)
        assert head == J.header(h, w, c, q) and len(head) == (334 if c == 1 else 629)
        segs, i = [], 2
        while i < len(head):
            assert head[i] == 0xFF
            length = struct.unpack(">H", head[i + 2:i + 4])[0]
            segs.append((head[i + 1], head[i + 4:i + 2 + length]))
            i += 2 + length
        assert i == len(head)
        assert [m for m, _ in segs] == [0xE0] + [0xDB] * (1 if c == 1 else 2) + [0xC0] + [0xC4] * (2 if c == 1 else 4) + [0xDD, 0xDA]
        assert segs[0][1] == b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00"
        sof = dict(segs)[0xC0]
        assert struct.unpack(">BHHB", sof[:6]) == (8, h, w, c)
        assert sof[6:] == (b"\x01\x11\x00" if c == 1 else b"\x01\x11\x00\x02\x11\x01\x03\x11\x01")
        assert dict(segs)[0xDD] == struct.pack(">H", (w + 7) // 8)
        assert dict(segs)[0xDA] == (b"\x01\x01\x00" if c == 1 else b"\x03\x01\x00\x02\x11\x03\x11") + b"\x00\x3f\x00"
        assert [p[0] for m, p in segs if m == 0xC4] == ([0x00, 0x10] if c == 1 else [0x00, 0x10, 0x01, 0x11])
    for bad in ((0, 8, 1), (8, 65536, 1), (8, 8, 2)):
        with pytest.raises(ValueError):
            ops.jpeg_header(*bad, quality=90)


def test_stuffing_and_padding_on_hand_made_bit_strings():
    assert J.pack_bits([0b101], [3]).tolist() == [0b10111111]                       # padded with 1-bits
    assert J.pack_bits([0xFF], [8]).tolist() == [0xFF]                              # a full byte is not padded
    assert J.pack_bits([], []).tolist() == []
    assert J.pack_bits([0b1, 0xFFFF, 0b0], [1, 16, 1]).tolist() == [0xFF, 0xFF, 0xBF]
    assert J.stuff([0xFF]).tolist() == [0xFF, 0]
    assert J.stuff([1, 0xFF, 0xFF, 2]).tolist() == [1, 0xFF, 0, 0xFF, 0, 2]
    assert J.stuff([0xFE, 0]).tolist() == [0xFE, 0]
    assert J.stuff(J.pack_bits([0b1111111], [7])).tolist() == [0xFF, 0]            # the padding itself makes an 0xFF
    # restart markers: the segment index mod 8, and the predictors start again
    frame = np.full((80, 16), 200, np.uint8)
    segs, scans, rst = J.parse(J.encode_frame(frame, 90))
    assert rst == [0xD0 + i % 8 for i in range(9)] and len(set(scans)) == 1


# ------------------------------------------------------------------------------------------------ the AVI file
def _clip(n, h, w, color, seed=3):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, h, w) + ((3,) if color else ()), dtype=np.uint8)


@pytest.mark.parametrize("color", (False, True))
def test_avi_structure_and_round_trip(restated_encoder, tmp_path, color):
    from video.io.backend_mjpeg import VideoMJPEG, VideoWriterMJPEG
    clip = _clip(7, 9, 17, color)
    path = tmp_path / "clip.avi"
    with VideoWriterMJPEG(path, (17, 9), 12.5, is_color=color, quality=75, batch=3) as writer:
        assert writer.shape == clip.shape[1:]
        for f in clip[:5]:
            writer.write_frame(f)
        assert [c[0] for c in restated_encoder] == [3]                             # a batch went out at the third frame
        writer.write_frames(clip[5:])
        assert writer.frames_written == 7
    assert [c[0] for c in restated_encoder] == [3, 2, 2] and all(c[1:] == (75, color) for c in restated_encoder)
    data = path.read_bytes()
    avi = J.parse_avi(data)
    want = J.encode(clip, 75)
    assert len(avi["frames"]) == 7 and [s for _, s in avi["frames"]] == [len(b) for b in want]
    for (at, size), b in zip(avi["frames"], want):
        assert data[at:at + size] == b and at % 2 == 0                             # chunks start on even offsets
        assert b[:2] == b"\xff\xd8" and b[-2:] == b"\xff\xd9"
    assert any(len(b) % 2 for b in want)                                           # (so the padding was exercised)
    assert avi["idx_cc"] == [b"00dc"] * 7
    for (flags, off, size), (at, s) in zip(avi["idx"][:, 1:].tolist(), avi["frames"]):
        assert flags == 0x10 and avi["movi_at"] + off + 8 == at and size == s
        assert data[avi["movi_at"] + off:avi["movi_at"] + off + 4] == b"00dc"
    assert data[avi["movi_at"]:avi["movi_at"] + 4] == b"movi"
    usec, _, _, flags, total, _, streams, _, width, height = avi["avih"][:10]
    assert (usec, flags, total, streams, width, height) == (80000, 0x10, 7, 1, 17, 9)
    assert avi["strh_type"] == b"vids" and avi["strh_handler"] == b"MJPG"
    assert avi["strh_scale_rate_start_length"] == (1000, 12500, 0, 7)
    assert avi["strf"][:6] == (40, 17, 9, 1, 24, struct.unpack("<I", b"MJPG")[0])
    with VideoMJPEG(path) as video:
        assert (video.frame_count, video.size, video.fps, video.is_color) == (7, (17, 9), 12.5, color)
        assert [video.get_frame_bytes(k) for k in range(7)] == want and video.get_frame_bytes(-1) == want[-1]
        with pytest.raises(IndexError):
            video.get_frame_bytes(7)
        try:
            import PIL  # noqa: F401
        except ImportError:
            with pytest.raises(ImportError, match="Pillow"):
                video.get_frame(0)
            return
        bound = [3, 3, 4] if color else [1]
        for k, frame in enumerate(video):
            ideal = J.ideal_decode(want[k])
            assert frame.shape == clip[k].shape and frame.dtype == np.uint8
            assert (np.abs(frame.astype(int) - ideal.astype(int)).reshape(-1, len(bound)).max(axis=0) <= bound).all()
        assert k == 6 and video[3].shape == clip[3].shape


def test_writer_refuses_what_the_composer_refuses(restated_encoder, tmp_path):
    from video.io.backend_mjpeg import VideoWriterMJPEG
    with VideoWriterMJPEG(tmp_path / "a.avi", (6, 5), 25, is_color=False) as writer:
        with pytest.raises(TypeError, match="frames are uint8"):
            writer.write_frame(np.zeros((5, 6), np.float32))
        with pytest.raises(ValueError, match="Cannot copy a color image into a monochrome video"):
            writer.write_frame(np.zeros((5, 6, 3), np.uint8))
        with pytest.raises(ValueError, match="in a video of size"):
            writer.write_frame(np.zeros((6, 5), np.uint8))
        with pytest.raises(ValueError, match="in a video of size"):
            writer.write_frames(np.zeros((2, 6, 5), np.uint8))
        assert writer.frames_written == 0
    assert J.parse_avi((tmp_path / "a.avi").read_bytes())["frames"] == []          # an empty file is still an AVI
    with pytest.raises(ValueError):
        writer.write_frame(np.zeros((5, 6), np.uint8))                             # closed
    for bad in (dict(quality=0), dict(batch=0), dict(codec="XVID"), dict(bitrate=10)):
        with pytest.raises((ValueError, TypeError)):
            VideoWriterMJPEG(tmp_path / "b.avi", (6, 5), 25, **bad)


def test_writer_stops_before_two_gib(restated_encoder, tmp_path, monkeypatch):
    from video.io import backend_mjpeg
    clip = _clip(6, 8, 8, False)
    sizes = [len(b) + (len(b) & 1) + 8 for b in J.encode(clip, 90)]
    # room for the header, four chunks and the index of four frames, and not one byte of a fifth
    monkeypatch.setattr(backend_mjpeg, "AVI_MAX_BYTES", 224 + sum(sizes[:4]) + 8 + 16 * 4 + sizes[4] - 1)
    writer = backend_mjpeg.VideoWriterMJPEG(tmp_path / "big.avi", (8, 8), 25, is_color=False, batch=6)
    with pytest.raises(OverflowError, match="AVI 1.0"):
        for f in clip:
            writer.write_frame(f)
    writer.close()
    data = (tmp_path / "big.avi").read_bytes()
    assert len(J.parse_avi(data)["frames"]) == 4 and len(data) <= backend_mjpeg.AVI_MAX_BYTES
    with backend_mjpeg.VideoMJPEG(tmp_path / "big.avi") as video:
        assert video.frame_count == 4


def test_reader_refuses_other_files(tmp_path, restated_encoder):
    from video.io.backend_mjpeg import VideoMJPEG, VideoWriterMJPEG
    with VideoWriterMJPEG(tmp_path / "ok.avi", (8, 8), 25, is_color=False) as writer:
        writer.write_frames(_clip(2, 8, 8, False))
    good = (tmp_path / "ok.avi").read_bytes()
    cut = good[:good.index(b"idx1")]
    variants = {"noriff": b"JUNK" + good[4:], "noidx": cut[:4] + struct.pack("<I", len(cut) - 8) + cut[8:],
                "codec": good.replace(b"MJPG", b"XVID"), "short": good[:10]}
    for name, data in variants.items():
        (tmp_path / name).write_bytes(data)
        with pytest.raises(ValueError):
            VideoMJPEG(tmp_path / name)


def test_write_video_and_load_any_video(restated_encoder, tmp_path):
    from video.io import file as vfile
    from video.io.memory import VideoMemory
    assert vfile.VideoFileWriter is vfile.VideoWriterMJPEG and vfile.VideoFile is vfile.VideoMJPEG
    clip = _clip(5, 10, 12, True)
    path = str(tmp_path / "w.avi")
    vfile.write_video(VideoMemory(clip, fps=30), path, quality=60, batch=2)
    assert [c[0] for c in restated_encoder] == [2, 2, 1]
    video = vfile.load_any_video(path)
    assert (video.frame_count, video.size, video.fps, video.is_color) == (5, (12, 10), 30, True)
    assert [video.get_frame_bytes(k) for k in range(5)] == J.encode(clip, 60)
    video.close()
    for pattern in ("a*.avi", "a?.avi", "a%d.avi"):
        with pytest.raises(NotImplementedError):
            vfile.load_any_video(pattern)


# ------------------------------------------------------------------------------------------------ the composer
@pytest.fixture
def restated_composer_ops(monkeypatch):
    import composer_checks as K
    from video import ops
    monkeypatch.setattr(ops, "compose_layers", lambda frames, layers, color=None, keep=False, stream=None:
                        K.compose_layers(frames, layers, color=color))
    monkeypatch.setattr(ops, "draw", lambda frames, commands, keep=False, stream=None: K.draw(frames, commands))


def _compose(sink, clip, color, **kwargs):
    from video.io.composer import VideoComposer
    h, w = clip.shape[1:3]
    vc = VideoComposer(sink, (w, h), 25, color, **kwargs)
    for f in clip:
        vc.set_frame(f)
        vc.add_rectangle((2, 2, 6, 5), "w")
    vc.close()
    return vc


@pytest.mark.parametrize("color", (False, True))
def test_composer_with_a_file_name(restated_encoder, restated_composer_ops, tmp_path, color):
    from video.io.backend_mjpeg import VideoMJPEG
    clip = _clip(5, 12, 14, color)
    frames = _compose(None, clip, color).frames
    for name in (str(tmp_path / "c.avi"), tmp_path / "p.avi"):                     # a str and an os.PathLike
        vc = _compose(name, clip, color, batch=2, quality=70)
        assert vc.frames_written == 5 and vc.sink.quality == 70
        with VideoMJPEG(name) as video:
            assert video.frame_count == 5 and video.size == (14, 12) and video.is_color == color
            assert [video.get_frame_bytes(k) for k in range(5)] == J.encode(frames, 70)
    with pytest.raises(TypeError):
        _compose(str(tmp_path / "x.avi"), clip, color, codec="XVID")               # the kwargs reach the writer


def test_composer_hands_device_stacks_to_a_write_frames_sink(restated_composer_ops, monkeypatch):
    """a sink with write_frames gets the flush's DeviceFrames; .frame, and host stacks, still go frame by frame"""
    from video import ops
    from video.io.composer import VideoComposer

    class Fake(ops.DeviceFrames):
        def __init__(self, arr):
            self.arr = arr
            ops.DeviceFrames.__init__(self, None, *arr.shape[:3], 3 if arr.ndim == 4 else 1)

        def download(self, stream=None):
            return self.arr

        def release(self):
            self.arr = None

    import composer_checks as K
    monkeypatch.setattr(ops, "compose_layers", lambda frames, layers, color=None, keep=False, stream=None:
                        Fake(K.compose_layers(frames.arr if isinstance(frames, Fake) else frames, layers, color=color)))
    monkeypatch.setattr(ops, "draw", lambda frames, commands, keep=False, stream=None:
                        Fake(K.draw(frames.arr, commands)))

    class Sink(object):
        def __init__(self):
            self.stacks, self.singles = [], []

        def write_frames(self, stack):
            assert isinstance(stack, ops.DeviceFrames)
            self.stacks.append(stack.arr.copy())

        def write_frame(self, frame):
            self.singles.append(frame.copy())

    clip = _clip(5, 12, 14, False)
    sink = Sink()
    vc = VideoComposer(sink, (14, 12), 25, False, batch=2)
    for k, f in enumerate(clip):
        vc.set_frame(f)
        vc.add_rectangle((2, 2, 6, 5), "w")
        if k == 4:
            assert vc.frame.shape == (12, 14)                  # reading .frame composes on the host side
    vc.close()
    want = _compose(None, clip, False).frames
    assert [len(s) for s in sink.stacks] == [2, 2] and len(sink.singles) == 1 and vc.frames_written == 5
    assert np.array_equal(np.concatenate(sink.stacks + [np.array(sink.singles)]), want)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_declaration_and_refusals():
    import ctypes as C
    from video import _hip
    text = open(os.path.join(ROOT, "include", "videoanalysis_hip.h")).read()
    assert "video/io/backend_opencv.py:240-242" in text and "video/io/file.py:50-64" in text
    res, args = _hip.SIGNATURES["va_jpeg_encode_u8"]
    assert res is C.c_int and len(args) == 14 and args[12] is C.c_int64
    L = _hip.load_library()
    fn = L.va_jpeg_encode_u8
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data
    ok = [p, 1, 8, 8, 1, p, p, 334, p, p, p, p, 64, None]

    def call(**change):
        names = ["frames", "n", "h", "w", "c", "qt", "head", "head_bytes", "sizes", "offsets", "totals", "out", "cap",
                 "stream"]
        a = list(ok)
        for k, v in change.items():
            a[names.index(k)] = v
        return fn(*a), L.va_last_error().decode()
    for change, word in ((dict(n=-1), "size"), (dict(h=0), "size"), (dict(w=0), "size"), (dict(cap=-1), "size"),
                         (dict(head_bytes=0), "size"), (dict(c=2), "channels"), (dict(c=4), "channels"),
                         (dict(frames=None), "NULL"), (dict(qt=None), "NULL"), (dict(head=None), "NULL"),
                         (dict(sizes=None), "NULL"), (dict(offsets=None), "NULL"), (dict(totals=None), "NULL"),
                         (dict(out=None), "NULL"), (dict(sizes=p + 4), "aligned"), (dict(offsets=p + 2), "aligned"),
                         (dict(totals=p + 1), "aligned"), (dict(h=65536), "16-bit"), (dict(w=70000), "16-bit")):
        rc, message = call(**change)
        assert rc == -22 and word in message, (change, rc, message)
    # the order of the checks: sizes, channels, NULL, alignment, 16 bits
    assert "size" in call(h=0, c=2)[1] and "channels" in call(c=2, frames=None)[1]
    assert "NULL" in call(frames=None, sizes=p + 4)[1] and "aligned" in call(sizes=p + 4, h=65536)[1]
    assert call(n=0, frames=None, c=3)[0] == 0                                      # n = 0 is VA_OK, nothing is looked at
    assert not buf.any()


# ------------------------------------------------------------------------------------------------ the header
def test_jpeg_math_header_on_the_host_under_sanitizers(fixture, tmp_path):
    """va_jpeg_math.h compiled for the host with -fsanitize=address,undefined into a stand-alone program that encodes
    fixture frames lane after lane; its tables and its entropy segments are the restatement's"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "llvm", "bin", "clang++")
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or (
        rocm_clang if os.path.exists(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler: neither g++, c++ or clang++ on the PATH nor %s" % rocm_clang
    exe = str(tmp_path / "jpeg_shim")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "video-analysis_amd", "csrc"),
                           os.path.join(ROOT, "tests", "jpeg_shim.cpp"), "-o", exe])
    names = ["noise_q100_37x53x3", "noise_q1_9x17x1", "noise_q50_7x64x3", "checker_80x16x1", "blockchecker_37x53x3",
             "lastzigzag_37x53x1", "zeros_1x1x3", "full_8x8x1", "flat_9x17x3", "noise_q90_80x16x3"]
    for name in names:
        frame, quality = fixture["frame_" + name], int(fixture["quality_" + name])
        h, w = frame.shape[:2]
        tables = J.quant_tables(quality)
        text = (struct.pack("<3i", h, w, 1 if frame.ndim == 2 else 3) + tables[0].astype(np.uint8).tobytes()
                + tables[1].astype(np.uint8).tobytes() + frame.tobytes())
        out = subprocess.run([exe], input=text, capture_output=True, check=True).stdout
        assert np.array_equal(np.frombuffer(out[:256], np.int32), J.ZIGZAG)
        assert np.array_equal(np.frombuffer(out[256:512], np.int32).reshape(8, 8), J.dct_matrix()[0])
        huff = np.frombuffer(out[512:512 + 4 * 544], np.uint32)
        for t in (0, 1):
            for sym, (code, length) in J.huffman_codes(*J.DHT[t]).items():
                assert huff[16 * t + sym] == (length << 16 | code)
            ac = huff[32 + 256 * t:32 + 256 * (t + 1)]
            codes = J.huffman_codes(*J.DHT[0x10 | t])
            assert all(ac[s] == ((codes[s][1] << 16 | codes[s][0]) if s in codes else 0) for s in range(256))
        at = 512 + 4 * 544
        for seg in J.frame_segments(frame, quality):
            size = struct.unpack("<i", out[at:at + 4])[0]
            assert out[at + 4:at + 4 + size] == seg.tobytes(), name
            at += 4 + size
        assert at == len(out)


def test_product_does_not_import_the_restatement():
    pkg = os.path.join(ROOT, "video-analysis_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                assert "jpeg_checks" not in open(os.path.join(dirpath, f)).read(), f
