"""Writes tests/golden/mjpeg_v1.npz: the small frames of the Motion-JPEG tests, the restatement's bytes for each
(tests/jpeg_checks.py, the definition of DESIGN.md §9, "Motion-JPEG") and Pillow's decode of those bytes.

Writing the fixture asserts the independent check, so that the tests need no Pillow: libjpeg decodes every stream
without error or warning to the right size and mode, and its pixels differ from the *ideal decode* of the same
coefficients (float64 IDCT and inverse colour matrix) by at most 1 per sample in monochrome -- the peak error IEEE
1180 allows an IDCT -- and by at most R 3, G 3, B 4 in colour, which is what 1 per component becomes through the
inverse matrix (1 + 1.402, 1 + 0.344 + 0.714, 1 + 1.772) and one rounding.  It also records how far the integer
transform is from rint(float64 DCT / Q).  Data only.  Run from the repository root: python tests/golden/make_golden_mjpeg.py
"""
import io
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_checks as J  # noqa: E402

SHAPES = ((1, 1), (8, 8), (9, 17), (7, 64), (80, 16), (37, 53))


def last_zigzag_blocks(h, w, amplitude):
    """blocks whose only non-zero AC coefficient is the last in zigzag order: amplitude * A[7][y] * A[7][x] around 128"""
    _, a = J.dct_matrix()
    block = np.rint(128 + amplitude * np.outer(a[7], a[7]))
    return np.clip(np.tile(block, ((h + 7) // 8, (w + 7) // 8))[:h, :w], 0, 255).astype(np.uint8)


def cases():
    """(name, frame, quality)"""
    rng = np.random.default_rng(20261019)
    out = []
    for h, w in SHAPES:
        for c in (1, 3):
            shape = (h, w) + ((3,) if c == 3 else ())
            tag = "%dx%dx%d" % (h, w, c)
            for q in (1, 50, 90, 100):
                out.append(("noise_q%d_%s" % (q, tag), rng.integers(0, 256, shape, dtype=np.uint8), q))
            out.append(("zeros_" + tag, np.zeros(shape, np.uint8), 90))
            out.append(("full_" + tag, np.full(shape, 255, np.uint8), 90))
            out.append(("flat_" + tag, np.full(shape, 100, np.uint8), 90))
            yy, xx = np.mgrid[:h, :w]
            board = np.where((yy + xx) % 2 == 0, 0, 255).astype(np.uint8)
            blocks = np.where((yy // 8 + xx // 8) % 2 == 0, 0, 255).astype(np.uint8)
            zz = last_zigzag_blocks(h, w, 500.0)
            for name, plane in (("checker", board), ("blockchecker", blocks), ("lastzigzag", zz)):
                frame = plane if c == 1 else np.stack([plane, plane, plane], axis=-1)
                out.append(("%s_%s" % (name, tag), frame, 100 if name != "lastzigzag" else 50))
    return out


def main():
    from PIL import Image
    store, names = {}, []
    worst = {"L": np.zeros(1, int), "RGB": np.zeros(3, int)}
    differ = total = 0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for name, frame, q in cases():
            data = J.encode_frame(frame, q)
            image = Image.open(io.BytesIO(data))
            image.load()
            mode = "L" if frame.ndim == 2 else "RGB"
            assert image.mode == mode and image.size == (frame.shape[1], frame.shape[0]), (name, image.mode, image.size)
            decoded = np.asarray(image)
            ideal = J.ideal_decode(data)
            err = np.abs(decoded.astype(int) - ideal.astype(int)).reshape(-1, len(worst[mode])).max(axis=0)
            bound = np.array([1]) if mode == "L" else np.array([3, 3, 4])
            assert (err <= bound).all(), "%s: Pillow is %s from the ideal decode (bound %s)" % (name, err, bound)
            worst[mode] = np.maximum(worst[mode], err)
            tables = J.quant_tables(q)
            for i, plane in enumerate(J.planes_of(frame)):
                fixed, ideal_q = J.forward(plane, tables[min(i, 1)]), J.float_quantised(plane, tables[min(i, 1)])
                assert np.abs(fixed - ideal_q).max() <= 1, name
                differ += int((fixed != ideal_q).sum())
                total += fixed.size
            names.append(name)
            store["frame_" + name] = frame
            store["bytes_" + name] = np.frombuffer(data, np.uint8)
            store["pillow_" + name] = decoded
            store["quality_" + name] = np.int32(q)
    store["names"] = np.array(names)
    store["pillow_worst_mono"] = worst["L"]
    store["pillow_worst_rgb"] = worst["RGB"]
    store["quantised_differ"] = np.array([differ, total], np.int64)
    path = os.path.join(HERE, "mjpeg_v1.npz")
    np.savez_compressed(path, **store)
    print("%d cases, %d bytes; Pillow vs ideal decode: mono %s, RGB %s; %d of %d quantised coefficients differ from "
          "rint(float64 DCT / Q), all by 1" % (len(names), os.path.getsize(path), worst["L"], worst["RGB"], differ, total))
    ff = sum(int((store["bytes_" + n][:-1] == 0xFF).sum()) for n in names if n.startswith("noise"))
    print("0xFF bytes in the noise streams (markers included):", ff)


if __name__ == "__main__":
    main()
