"""Writes tests/golden/mjpeg_encode_sampled_v1.npz: the pinned 4:2:2 and 4:2:0 streams of DESIGN.md §9, "Subsampled
Motion-JPEG encoding" (tests/jpeg_sampled_encode_checks.py states the format; the bytes are
jpeg_subsampled_checks.encode_frame's).

The two layouts x the shapes 1x1, 8x8, 16x16, 17x17, 18x34, 9x17, 7x64, 37x53, 80x16, 16x48 and 33x16 x {noise, a
ramp, all 0, all 255} x the qualities 1, 50, 90 and 100, and per layout a checkerboard of single pixels and one of
2 x 2-pixel cells (red and blue, 18x34, quality 100): the box average flattens the chroma of the first and leaves
that of the second (both asserted).  Stored are each frame once, every stream, and Pillow's decode of every stream as
its difference from jpeg_subsampled_checks.ideal_decode of the same bytes.

Writing the fixture asserts, for every stream and with no case left out, that Pillow opens and decodes it without an
error or a warning to the frame's size, and that its pixels are within R 3, G 3, B 4 of the ideal decode.  The maxima
seen are stored and printed.  Data only.
Run from the repository root: python tests/golden/make_golden_mjpeg_encode_sampled.py"""
import io
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_decode_checks as D  # noqa: E402
import jpeg_sampled_encode_checks as E  # noqa: E402
import jpeg_subsampled_checks as S  # noqa: E402


def pillow_decode(data, name):
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        image = Image.open(io.BytesIO(data))
        image.load()
        assert image.format == "JPEG" and image.mode == "RGB", name
        return np.asarray(image.convert("RGB"))


def main():
    rng = np.random.default_rng(20261020)
    frames = {}
    for h, w in E.SHAPES:
        for content in E.CONTENTS:
            frames["%s_%dx%d" % (content, h, w)] = E.frame_of(content, h, w, rng)
    for content in ("checker1", "checker2"):
        frames["%s_%dx%d" % ((content,) + E.CHECKER_SHAPE)] = E.frame_of(content, *E.CHECKER_SHAPE, rng)
    names, frame_of, sampling, quality, streams, diffs = [], [], [], [], [], []
    worst, worst_base = np.zeros(3, int), np.zeros(3, int)
    for layout, hv in E.LAYOUTS:
        todo = [(key, q) for key in frames if not key.startswith("checker") for q in E.QUALITIES]
        todo += [(key, 100) for key in frames if key.startswith("checker")]
        for key, q in todo:
            frame = frames[key]
            name = "%s_q%d_%s" % (key, q, layout)
            data = S.encode_frame(frame, q, hv, ri=None)
            head = D.parse_header(data, sampling="any")
            assert head["sampling"] == hv and head["ri"] == -(-frame.shape[1] // (8 * hv[0])) and len(data) > 629, name
            seen = pillow_decode(data, name)
            assert seen.shape == frame.shape and seen.dtype == np.uint8, name
            d = seen.astype(np.int16) - S.ideal_decode(data, head).astype(np.int16)
            err = np.abs(d).reshape(-1, 3).max(axis=0)
            assert (err <= E.BOUND).all(), (name, err)
            worst = np.maximum(worst, err)
            if not key.startswith("checker"):
                worst_base = np.maximum(worst_base, err)
            names.append(name)
            frame_of.append(key)
            sampling.append(hv)
            quality.append(q)
            streams.append(data)
            diffs.append(d.astype(np.int8).ravel())
    assert len(names) == 2 * (len(E.SHAPES) * len(E.CONTENTS) * len(E.QUALITIES) + 2) == 356
    by_name = dict(zip(names, streams))

    def flat(name, comp):
        data = by_name[name]
        return (D.decode_coefficients(data, D.parse_header(data, sampling="any"))[0][comp][:, :, 1:] == 0).all()
    for layout, _ in E.LAYOUTS:                             # the pixel checkerboard's chroma is flat, its luma is not
        assert flat("checker1_18x34_q100_" + layout, 1) and not flat("checker1_18x34_q100_" + layout, 0)
        assert not flat("checker2_18x34_q100_" + layout, 1)
    store = dict(names=np.array(names), frame_of=np.array(frame_of), sampling=np.array(sampling, np.int64),
                 quality=np.array(quality, np.int64), blob=np.frombuffer(b"".join(streams), np.uint8),
                 offsets=np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.int64),
                 pillow_diff=np.concatenate(diffs), frame_names=np.array(list(frames)),
                 frame_shapes=np.array([f.shape[:2] for f in frames.values()], np.int64),
                 frame_blob=np.concatenate([f.ravel() for f in frames.values()]),
                 pillow_worst_rgb=worst.astype(np.int64), pillow_worst_rgb_base=worst_base.astype(np.int64))
    path = os.path.join(HERE, "mjpeg_encode_sampled_v1.npz")
    np.savez_compressed(path, **store)
    print("%d cases, %d stream bytes, %d bytes of fixture" % (len(names), len(store["blob"]), os.path.getsize(path)))
    print("Pillow vs the ideal decode: RGB at most %s on the %d base cases, %s on all" % (worst_base, len(names) - 4, worst))


if __name__ == "__main__":
    main()
