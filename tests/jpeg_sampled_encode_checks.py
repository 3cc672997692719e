"""The 4:2:2 and 4:2:0 streams of DESIGN.md §9, "Subsampled Motion-JPEG encoding": a pinned format.  The definition is,
byte for byte, what jpeg_subsampled_checks.encode_frame(frame, quality, sampling, ri=None) writes for a three-component
frame and sampling (H, V) = (2, 1) or (2, 2) -- that function was written to make decoder inputs, and its bytes are now
what va_jpeg_encode_sampled_u8 and ops.jpeg_encode(sampling=...) must write:

  SOF0 gives the luma component H << 4 | V and Cb, Cr 0x11; an MCU is the H V luma blocks in row-major order, Cb, Cr;
  the grid is my = ceil(h / 8 V) by mx = ceil(w / 8 H) MCUs, DRI is mx (one restart interval per MCU row, RSTm between
  them); the header stays 629 bytes.  Y is padded to 8 V my x 8 H mx by repeating its last row and column.  Cb and Cr
  are computed per pixel with the pinned colour formula, padded to a multiple of V x H by repeating the edge, box-
  averaged as (sum of the H V samples + H V / 2) // (H V), and the averaged plane, ceil(h / V) x ceil(w / H), is padded
  to 8 my x 8 mx by repeating its own last row and column.  Transform, quantiser (table 0 for Y, 1 for Cb and Cr),
  Huffman tables, DC prediction per component from 0 at every restart, padding, stuffing and EOI are jpeg_checks'.

Here: the encoder over stacks, the chroma plane on its own (for hand-made checks), and the reader of the fixture
tests/golden/mjpeg_encode_sampled_v1.npz.  Nothing here imports the package."""
import numpy as np

import jpeg_subsampled_checks as S

LAYOUTS = (("422", (2, 1)), ("420", (2, 2)))
SHAPES = ((1, 1), (8, 8), (16, 16), (17, 17), (18, 34), (9, 17), (7, 64), (37, 53), (80, 16), (16, 48), (33, 16))
CONTENTS = ("noise", "ramp", "zeros", "full")
QUALITIES = (1, 50, 90, 100)
CHECKER_SHAPE = (18, 34)                # the two checkerboards, at quality 100
BOUND = (3, 3, 4)                       # R, G, B: a decoder's distance from jpeg_subsampled_checks.ideal_decode


def encode(frames, quality=90, sampling=(2, 2)):
    """the files of a stack (n, h, w, 3) as a list of bytes"""
    frames = np.asarray(frames)
    assert frames.ndim == 4
    return [S.encode_frame(f, quality, tuple(sampling), ri=None) for f in frames]


def packed(files):
    """(blob, offsets) as ops.jpeg_encode(ret_packed=True) returns them"""
    offsets = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)
    return np.frombuffer(b"".join(files), np.uint8), offsets


def averaged_plane(plane, sampling, my, mx):
    """a Cb or Cr plane (h, w) of per-pixel samples -> the (8 my, 8 mx) plane the chroma blocks are cut from"""
    hh, vv = sampling
    h, w = plane.shape
    pad = lambda p, rows, cols: np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")
    p = pad(np.asarray(plane, np.int64), -(-h // vv) * vv, -(-w // hh) * hh)
    total = p.reshape(p.shape[0] // vv, vv, p.shape[1] // hh, hh).sum(axis=(1, 3))
    return pad((total + hh * vv // 2) // (hh * vv), 8 * my, 8 * mx)


def frame_of(content, h, w, rng):
    """the fixture's pictures: `rng` is drawn from for noise only"""
    if content == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if content == "ramp":
        yy, xx = np.mgrid[:h, :w]
        return np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1),
                         (xx + yy) * 255 // max(h + w - 2, 1)], axis=-1).astype(np.uint8)
    if content in ("zeros", "full"):
        return np.full((h, w, 3), 0 if content == "zeros" else 255, np.uint8)
    cell = {"checker1": 1, "checker2": 2}[content]
    yy, xx = np.mgrid[:h, :w]
    on = ((yy // cell + xx // cell) % 2).astype(bool)
    return np.where(on[:, :, None], np.array([255, 0, 0], np.uint8), np.array([0, 0, 255], np.uint8))


def fixture_cases(path):
    """[(name, (H, V), quality, frame, the pinned bytes, Pillow's difference)] of tests/golden/mjpeg_encode_sampled_v1.npz,
    and the archive.  A frame is stored once per (content, shape); Pillow's pixels as their int16 difference from
    jpeg_subsampled_checks.ideal_decode of the bytes, which pillow_pixels(case) adds again."""
    z = np.load(path, allow_pickle=False)
    frames, at = {}, 0
    for key, (h, w) in zip(z["frame_names"], z["frame_shapes"]):
        n = int(h) * int(w) * 3
        frames[str(key)] = z["frame_blob"][at:at + n].reshape(int(h), int(w), 3)
        at += n
    out, at = [], 0
    for k, name in enumerate(z["names"]):
        data = z["blob"][z["offsets"][k]:z["offsets"][k + 1]].tobytes()
        frame = frames[str(z["frame_of"][k])]
        n = frame.size
        diff = z["pillow_diff"][at:at + n].reshape(frame.shape).astype(np.int16)
        at += n
        out.append((str(name), tuple(int(v) for v in z["sampling"][k]), int(z["quality"][k]), frame, data, diff))
    return out, z


def groups(cases):
    """{(shape, layout, quality): [case]}: the stacks one encoder call takes"""
    out = {}
    for case in cases:
        out.setdefault((case[3].shape, case[1], case[2]), []).append(case)
    return out


def pillow_pixels(case):
    """what Pillow decoded from a case's bytes when the fixture was written"""
    return (S.ideal_decode(case[4]).astype(np.int16) + case[5]).astype(np.uint8)
