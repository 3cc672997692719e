"""Motion-JPEG in an AVI container: the package's video file backend (the reference's are `backend_opencv.py` and
`backend_ffmpeg.py`, over cv2.VideoWriter and an ffmpeg child process; neither exists where this package runs).

`VideoWriterMJPEG` follows the reference writers' protocol (`shape`, `write_frame`, `frames_written`, `close`, the
context manager) and adds `write_frames` for a whole stack, host or device.  Frames are buffered, `batch` at a time
encoded by one `ops.jpeg_encode` call ("Motion-JPEG": one baseline JFIF file per frame) and streamed
into a RIFF AVI 1.0 file:

    RIFF 'AVI '  LIST 'hdrl' ( avih  LIST 'strl' ( strh 'vids' / 'MJPG'   strf BITMAPINFOHEADER 'MJPG', 24 bit ) )
                 LIST 'movi' ( '00dc' chunk per frame, padded to even length )
                 idx1        ( per frame: '00dc', AVIIF_KEYFRAME, offset from 'movi', size )

The sizes and the frame count are written on `close()`.  AVI 1.0 holds less than 2 GiB: a frame that would take the
file beyond 2^31 - 1 bytes raises before anything of it is written, and the file closes as a valid one.

`VideoMJPEG` reads such a file back as a seekable `VideoBase`: any AVI 1.0 with one MJPG video stream and an idx1.
`get_frame_bytes(i)` is the stored JFIF file; `get_frame(i)` decodes it through Pillow, imported when first needed.
Host code only: the encoder is `ops.jpeg_encode`, looked up on `video.ops` at each flush.
"""
import os
import struct

import numpy as np

from .. import ops
from .base import VideoBase

AVI_MAX_BYTES = 2 ** 31 - 1
_AVIF_HASINDEX = 0x10
_AVIIF_KEYFRAME = 0x10
_HEADER_BYTES = 224                     # RIFF .. the 'movi' tag: what close() rewrites
_MOVI_TAG_AT = _HEADER_BYTES - 4


def _rate_scale(fps):
    """dwRate / dwScale of a frame rate: the rate itself when it is whole, else thousandths"""
    fps = float(fps)
    if not (fps > 0 and fps < 1e6):
        raise ValueError("fps must be positive, got %r" % (fps,))
    return (int(fps), 1) if fps == int(fps) else (int(round(fps * 1000)), 1000)


def _avi_header(size, fps, frames, movi_bytes, idx_bytes, largest):
    """the first 224 bytes of the file; movi_bytes: the chunks of the movi list, idx_bytes: the idx1 payload"""
    width, height = size
    rate, scale = _rate_scale(fps)
    avih = struct.pack("<14I", int(round(1e6 * scale / rate)), int(largest * rate / scale), 0, _AVIF_HASINDEX, frames,
                       0, 1, largest, width, height, 0, 0, 0, 0)
    strh = struct.pack("<4s4sIHHIIIIIIII4h", b"vids", b"MJPG", 0, 0, 0, 0, scale, rate, 0, frames, largest,
                       0xFFFFFFFF, 0, 0, 0, width, height)
    strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, b"MJPG", width * height * 3, 0, 0, 0, 0)
    strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
    hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
    riff_bytes = 4 + 8 + len(hdrl) + 8 + 4 + movi_bytes + 8 + idx_bytes
    out = (b"RIFF" + struct.pack("<I", riff_bytes) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl
           + b"LIST" + struct.pack("<I", 4 + movi_bytes) + b"movi")
    assert len(out) == _HEADER_BYTES
    return out


class VideoWriterMJPEG(object):
    """writes uint8 frames into a Motion-JPEG AVI file, `batch` frames per encoder call"""

    def __init__(self, filename, size, fps, is_color=True, quality=90, batch=32, sampling=(1, 1),
                 optimize=False, **kwargs):
        """`size` = (width, height); `quality` 1 .. 100 (the IJG scale); `sampling` of a colour video: (1, 1) /
        "4:4:4", (2, 1) / "4:2:2" or (2, 2) / "4:2:0" ("Subsampled Motion-JPEG encoding"); `optimize`:
        every encoder call writes its `batch` frames with Huffman tables made for them ("Optimised
        Huffman tables"), so the file's frames share their header in runs of `batch`; further keyword arguments --
        the codec and bitrate of the reference's writers -- have no meaning here and are refused"""
        if kwargs:
            raise TypeError("VideoWriterMJPEG: unknown arguments %s (the codec is MJPG; quality, batch, sampling and "
                            "optimize are what can be set)" % ", ".join(sorted(kwargs)))
        self.sampling = ops.jpeg_sampling(sampling, 3 if is_color else 1, "VideoWriterMJPEG")
        self.optimize = ops.jpeg_optimize_flag(optimize, "VideoWriterMJPEG")
        if batch < 1:
            raise ValueError("batch must be positive")
        self.filename = os.fspath(filename)
        self.size = (int(size[0]), int(size[1]))
        if not (1 <= self.size[0] <= ops.JPEG_MAX_SIDE and 1 <= self.size[1] <= ops.JPEG_MAX_SIDE):
            raise ValueError("frame sides are 1 .. %d, got %r" % (ops.JPEG_MAX_SIDE, self.size))
        self.fps, self.is_color, self.batch = fps, bool(is_color), int(batch)
        _rate_scale(fps)
        ops.jpeg_tables(quality)                  # (raises for a quality outside 1 .. 100)
        self.quality = int(quality)
        self.frames_written = 0
        self._buffer = []
        self._index = []                          # (offset from the 'movi' tag, size) per frame
        self._largest = 0
        self._file = open(self.filename, "wb")
        self._file.write(_avi_header(self.size, self.fps, 0, 0, 0, 0))
        self._at = _HEADER_BYTES

    @property
    def shape(self):
        """the shape of one frame"""
        return (self.size[1], self.size[0]) + ((3,) if self.is_color else ())

    # ------------------------------------------------------------------------------------------ frames in
    def _check(self, shape, dtype, stack):
        if dtype != np.uint8:
            raise TypeError("frames are uint8, got %s" % dtype)
        if tuple(shape[1:] if stack else shape) != self.shape:
            if not self.is_color and len(shape) == (4 if stack else 3):
                raise ValueError("Cannot copy a color image into a monochrome video.")
            raise ValueError("a frame of shape %r in a video of size %r" % (tuple(shape[1:] if stack else shape),
                                                                             self.size))

    def write_frame(self, frame):
        """buffers one (h, w[, 3]) uint8 frame (a copy of it); every `batch` frames go to the encoder"""
        if self._file is None:
            raise ValueError("the video file is closed")
        frame = np.asarray(frame)
        self._check(frame.shape, frame.dtype, False)
        self._buffer.append(np.array(frame, copy=True))
        self.frames_written += 1
        if len(self._buffer) >= self.batch:
            self._flush()

    def write_frames(self, frames):
        """a whole stack at once: an (n, h, w[, 3]) uint8 array or an ops.DeviceFrames, which is encoded where it
        is (it stays the caller's) -- only compressed bytes cross to the host"""
        if self._file is None:
            raise ValueError("the video file is closed")
        device = isinstance(frames, ops.DeviceFrames)
        if not device:
            frames = np.asarray(frames)
        self._check(frames.shape, np.dtype(np.uint8) if device else frames.dtype, True)
        self._flush()
        count = frames.n if device else len(frames)
        if count:
            self._encode(frames)
        self.frames_written += count

    def _flush(self):
        if self._buffer:
            stack, self._buffer = np.stack(self._buffer), []
            self._encode(stack)

    def _encode(self, stack):
        layout = {} if self.sampling == (1, 1) else {"sampling": self.sampling}        # (1, 1): the call as it was
        if self.optimize:
            layout["optimize"] = True
        blob, offsets = ops.jpeg_encode(stack, quality=self.quality, color=self.is_color, ret_packed=True,
                                        **layout)
        blob = np.asarray(blob, np.uint8)
        for k in range(len(offsets) - 1):
            data = blob[offsets[k]:offsets[k + 1]]
            padded = len(data) + (len(data) & 1)
            # what the file holds once this chunk and the index are in: it must stay an AVI 1.0 file
            if self._at + 8 + padded + 8 + 16 * (len(self._index) + 1) > AVI_MAX_BYTES:
                raise OverflowError("frame %d would take %s beyond %d bytes (AVI 1.0); close() keeps the %d frames "
                                    "written so far" % (len(self._index), self.filename, AVI_MAX_BYTES, len(self._index)))
            self._file.write(b"00dc" + struct.pack("<I", len(data)))
            self._file.write(data.tobytes())
            if padded != len(data):
                self._file.write(b"\0")
            self._index.append((self._at - _MOVI_TAG_AT, len(data)))
            self._largest = max(self._largest, len(data))
            self._at += 8 + padded

    # ------------------------------------------------------------------------------------------ closing
    def close(self):
        """encodes what is buffered, writes idx1 and the final header"""
        if self._file is None:
            return
        try:
            self._flush()
        finally:
            f, self._file = self._file, None
            with f:
                idx = b"".join(struct.pack("<4sIII", b"00dc", _AVIIF_KEYFRAME, off, size) for off, size in self._index)
                f.write(b"idx1" + struct.pack("<I", len(idx)) + idx)
                f.seek(0)
                f.write(_avi_header(self.size, self.fps, len(self._index), self._at - _HEADER_BYTES, len(idx),
                                    self._largest))
            self.frames_written = len(self._index)

    def __enter__(self):
        return self

    def __exit__(self, e_type, e_value, e_traceback):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _chunks(data, start, end):
    """(fourcc, offset of the data, size) of the RIFF chunks of a byte range"""
    i = start
    while i + 8 <= end:
        size = struct.unpack("<I", data[i + 4:i + 8])[0]
        if i + 8 + size > end:
            raise ValueError("a chunk at byte %d leaves its list" % i)
        yield data[i:i + 4], i + 8, size
        i += 8 + size + (size & 1)


class VideoMJPEG(VideoBase):
    """a Motion-JPEG AVI 1.0 file (one MJPG video stream and an idx1) as a seekable video"""

    seekable = True

    DEVICE_BATCH = 32                    # frames per decoder call with parameters={"decoder": "device"}

    def __init__(self, filename, parameters=None):
        """parameters: {"decoder": "pillow"} (the default: get_frame decodes one frame on the host through Pillow) or
        {"decoder": "device"}: get_frame and iteration serve frames from batches of DEVICE_BATCH frames decoded by
        one ops.jpeg_decode call each, through a cache of one batch.  The device decoder (also behind get_frames
        and get_device_frames) reads monochrome and 4:4:4 files and the 4:2:0 and 4:2:2 files of cameras and other
        encoders; every frame of the file must have one shape"""
        parameters = dict(parameters or {})
        self._decoder = parameters.pop("decoder", "pillow")
        if self._decoder not in ("pillow", "device"):
            raise ValueError("the decoder is 'pillow' or 'device', got %r" % (self._decoder,))
        self._batch_start, self._batch = 0, None
        self.filename = os.fspath(filename)
        self._file = open(self.filename, "rb")
        try:
            fmt = self._read_structure()
        except Exception:
            self._file.close()
            raise
        super(VideoMJPEG, self).__init__(**fmt)

    def _read_structure(self):
        f = self._file
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"AVI ":
            raise ValueError("%s is not a RIFF AVI file" % self.filename)
        f.seek(0, os.SEEK_END)
        end = min(f.tell(), 8 + struct.unpack("<I", head[4:8])[0])
        # the top-level chunks, read without their payloads
        top, at = {}, 12
        while at + 8 <= end:
            f.seek(at)
            cc, size = struct.unpack("<4sI", f.read(8))
            name = cc + f.read(4) if cc == b"LIST" else cc
            top.setdefault(name, (at + 8, size))
            at += 8 + size + (size & 1)
        for name in (b"LISThdrl", b"LISTmovi", b"idx1"):
            if name not in top:
                raise ValueError("%s: no %s chunk (an AVI 1.0 file with an index is needed)"
                                 % (self.filename, name.decode()))
        f.seek(top[b"LISThdrl"][0])
        hdrl = f.read(top[b"LISThdrl"][1])
        avih, streams = None, []
        for cc, at, size in _chunks(hdrl, 4, len(hdrl)):
            if cc == b"avih":
                avih = struct.unpack("<14I", hdrl[at:at + 56])
            elif cc == b"LIST" and hdrl[at:at + 4] == b"strl":
                streams.append(dict((c, hdrl[a:a + s]) for c, a, s in _chunks(hdrl, at + 4, at + size)))
        if avih is None or len(streams) != 1 or b"strh" not in streams[0] or b"strf" not in streams[0]:
            raise ValueError("%s: one video stream is needed, found %d stream(s)" % (self.filename, len(streams)))
        strh, strf = streams[0][b"strh"], streams[0][b"strf"]
        if strh[:4] != b"vids" or len(strf) < 40 or strf[16:20].upper() not in (b"MJPG",):
            raise ValueError("%s: the stream is not MJPG video (%r / %r)" % (self.filename, strh[:4], strf[16:20]))
        scale, rate = struct.unpack("<II", strh[20:28])
        width, height = struct.unpack("<ii", strf[4:12])
        f.seek(top[b"idx1"][0])
        idx = np.frombuffer(f.read(top[b"idx1"][1] // 16 * 16), np.dtype("<u4")).reshape(-1, 4)
        idx = idx[idx[:, 0] == struct.unpack("<I", b"00dc")[0]]
        # idx1 offsets count from the 'movi' tag, or, in files of some writers, from the start of the file
        movi_tag = top[b"LISTmovi"][0]
        base = movi_tag
        if len(idx):
            f.seek(movi_tag + int(idx[0, 2]))
            if f.read(4) != b"00dc":
                base = 0
        self._frames = [(base + int(off) + 8, int(size)) for _, _, off, size in idx]
        for pos, size in self._frames[:1] + self._frames[-1:]:
            f.seek(pos - 8)
            if f.read(8) != b"00dc" + struct.pack("<I", size):
                raise ValueError("%s: idx1 does not point at the stream's chunks" % self.filename)
        self._mode = None
        is_color = True
        if self._frames:                      # the first frame's SOF0 says whether the stream is monochrome
            is_color = self._components(self.get_frame_bytes(0)) != 1
        fps = rate / scale if scale else 25
        return dict(size=(width, abs(height)), frame_count=len(self._frames), fps=int(fps) if fps == int(fps) else fps,
                    is_color=is_color)

    @staticmethod
    def _components(data):
        i = 2
        while i + 4 <= len(data) and data[i] == 0xFF:
            marker, length = data[i + 1], struct.unpack(">H", data[i + 2:i + 4])[0]
            if marker in (0xC0, 0xC1, 0xC2):
                return data[i + 9]
            if marker == 0xDA:
                break
            i += 2 + length
        raise ValueError("a frame without a frame header")

    def get_frame_bytes(self, index):
        """the stored JFIF file of frame `index`"""
        index = index + len(self._frames) if index < 0 else index
        if index < 0 or index >= len(self._frames):
            raise IndexError("frame %d is out of range" % index)
        if self._file is None:
            raise ValueError("the video file is closed")
        pos, size = self._frames[index]
        self._file.seek(pos)
        return self._file.read(size)

    def _streams(self, start, stop):
        count = len(self._frames)
        start = 0 if start is None else start + count if start < 0 else start
        stop = count if stop is None else stop + count if stop < 0 else stop
        if not 0 <= start <= stop <= count:
            raise IndexError("frames %r .. %r are out of range (the video has %d)" % (start, stop, count))
        return [self.get_frame_bytes(i) for i in range(start, stop)]

    def get_frames(self, start=None, stop=None):
        """the frames start .. stop - 1 as one uint8 array (n, h, w) or (n, h, w, 3), decoded on the device by one
        ops.jpeg_decode call (no Pillow); the frames are as stored, without `_process_frame`"""
        from .. import ops
        return ops.jpeg_decode(self._streams(start, stop), color=self.is_color)

    def get_device_frames(self, start=None, stop=None):
        """the frames start .. stop - 1 as an ops.DeviceFrames that stays on the device (the caller releases it): only
        the stored bytes cross the bus"""
        from .. import ops
        return ops.jpeg_decode(self._streams(start, stop), color=self.is_color, keep=True)

    def _device_frame(self, index):
        count = len(self._frames)
        index = index + count if index < 0 else index
        if index < 0 or index >= count:
            raise IndexError("frame %d is out of range" % index)
        if self._batch is None or not self._batch_start <= index < self._batch_start + len(self._batch):
            start = index - index % self.DEVICE_BATCH
            self._batch = None
            self._batch = self.get_frames(start, min(start + self.DEVICE_BATCH, count))
            self._batch_start = start
        return self._process_frame(self._batch[index - self._batch_start].copy())

    def get_frame(self, index):
        if self._decoder == "device":
            return self._device_frame(index)
        data = self.get_frame_bytes(index)
        try:
            from PIL import Image
        except ImportError:
            raise ImportError("decoding a Motion-JPEG frame needs Pillow (PIL), which is not installed; "
                              "get_frame_bytes(i) returns the stored JPEG file without it")
        import io
        image = Image.open(io.BytesIO(data))
        frame = np.asarray(image.convert("RGB" if self.is_color else "L"))
        return self._process_frame(frame)

    def close(self):
        if self._file is not None:
            self._file.close()
            self._file = None

    def __enter__(self):
        return self

    def __exit__(self, e_type, e_value, e_traceback):
        self.close()
        return False
