"""Writes tests/golden/mjpeg_optimized_v1.npz for DESIGN.md §9, "Optimised Huffman tables"
(tests/jpeg_optimize_checks.py states the definition and reads the archive).

1  The libjpeg pin.  Pillow (libjpeg) writes colour pictures of 8x8, 33x47, 64x96 and 200x312 at the qualities 10,
   50, 75, 90 and 100 in 4:4:4, 4:2:2 and 4:2:0 with optimize=True, and two monochrome ones.  Stored are the symbol
   counts recovered from each file (jpeg_optimize_checks.file_counts) and the file's own tables.  200x312 at quality
   100 in 4:4:4 is left out: Pillow refuses to write it ("Suspension not allowed here").  Any other refusal fails
   the run, the tables of every file must be what gen_optimal_table makes of its counts, and there are at least 230.
2  Chosen counts (jpeg_optimize_checks.chosen_counts, drawn again from their seed by the reader) with the
   restatement's tables.
3  Small calls of every layout with the restatement's optimised streams and Pillow's decode of each stream, which
   must equal its decode of the plain stream of the same frame.  A stack is stored once; Pillow's pixels as their int8
   difference from jpeg_subsampled_checks.ideal_decode of the same bytes.
4  Pillow's own plain and optimised sizes of the benchmark's two 1080p pictures (tools/bench_mjpeg.py --optimize).

A table is stored as the code length of each of its 256 symbols: BITS is their histogram and HUFFVAL lists the symbols
by length, then value, which the run asserts for every table it stores.  Data only.
Run from the repository root: python tests/golden/make_golden_mjpeg_optimized.py"""
import io
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_optimize_checks as O  # noqa: E402
import jpeg_subsampled_checks as S  # noqa: E402

PIN_SIZES = ((8, 8), (33, 47), (64, 96), (200, 312))
PIN_QUALITIES = (10, 50, 75, 90, 100)
PIN_SAMPLINGS = (("444", 0), ("422", 1), ("420", 2))
PIN_REFUSED = ("200x312", 100, "444")
CALLS = ((1, 7, 9, 90), (3, 17, 33, 90), (1, 37, 53, 50), (3, 16, 16, 100), (1, 1, 1, 1))     # n, h, w, quality


def picture(h, w, c, rng):
    """a smooth pattern with an edge and noise of growing strength: many different symbols"""
    yy, xx = np.mgrid[:h, :w]
    base = 128 + 70 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + 40 * (xx > w // 2)
    planes = [np.clip(np.roll(base, 3 * k, axis=0) + rng.normal(0, 1 + 24 * yy / max(h - 1, 1), (h, w)), 0, 255)
              for k in range(c)]
    return np.stack(planes, axis=-1).astype(np.uint8) if c == 3 else planes[0].astype(np.uint8)


def scene(h, w, c, rng, noise):
    """frame 0 of tools/bench_mjpeg.py's scene"""
    if noise:
        return rng.integers(0, 256, (h, w) + ((3,) if c == 3 else ()), dtype=np.uint8)
    yy, xx = np.mgrid[:h, :w]
    base = 128 + 60 * np.sin(xx / 97.0) * np.cos(yy / 71.0)
    for _ in range(12):
        cx, cy, r = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(h / 40, h / 10)
        base[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] += rng.uniform(-60, 60)
    plane = np.clip(base + rng.integers(-4, 5, (h, w)), 0, 255).astype(np.uint8)
    return plane if c == 1 else np.stack([plane, np.roll(plane, 5, axis=0), 255 - plane], axis=-1)


def pillow_write(frame, quality, subsampling, optimize):
    from PIL import Image
    buf = io.BytesIO()
    kwargs = {} if frame.ndim == 2 else {"subsampling": subsampling}
    Image.fromarray(frame).save(buf, "JPEG", quality=quality, optimize=optimize, **kwargs)
    return buf.getvalue()


def pillow_decode(data, name):
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        image = Image.open(io.BytesIO(data))
        image.load()
        assert image.format == "JPEG", name
        return np.asarray(image)


def packed_tables(tables):
    """[(BITS, HUFFVAL)] as jpeg_optimize_checks.unpacked_tables reads them: the code length of every symbol, and in
    full the tables that the lengths do not give back (the limit to 16 bits keeps the order by the unlimited size)"""
    lengths, odd, full = np.zeros((len(tables), 256), np.uint8), [], []
    for k, (bits, vals) in enumerate(tables):
        for sym, n in O.code_lengths(bits, vals).items():
            lengths[k, sym] = n
        if not np.array_equal(O.table_from_lengths(lengths[k]), O.table_bytes(bits, vals)):
            odd.append(k)
            full.append(O.table_bytes(bits, vals))
    return {"lengths": lengths, "odd": np.array(odd, np.int32),
            "full": np.stack(full) if full else np.zeros((0, O.TABLE_BYTES), np.uint8)}


def main():
    rng = np.random.default_rng(20261020)
    # ---------------------------------------------------------------- 1: the libjpeg pin
    pin_names, pin_tables_of, pin_counts, pin_lengths = [], [], [], []

    def pin(name, data, c):
        freq, tables = O.file_counts(data)
        t = 2 if c == 1 else 4
        for k in range(t):
            want = O.gen_optimal_table(freq[k >> 1, k & 1])
            assert (list(want[0]), list(want[1])) == (list(tables[O.KEYS[k]][0]), list(tables[O.KEYS[k]][1])), (name, k)
            pin_lengths.append(tables[O.KEYS[k]])
        pin_names.append(name)
        pin_tables_of.append(t)
        pin_counts.append(freq.reshape(4, 256)[:t])
    for h, w in PIN_SIZES:
        frame = picture(h, w, 3, rng)
        for q in PIN_QUALITIES:
            for layout, sub in PIN_SAMPLINGS:
                name = "%dx%d_q%d_%s" % (h, w, q, layout)
                if ("%dx%d" % (h, w), q, layout) == PIN_REFUSED:
                    continue
                pin(name, pillow_write(frame, q, sub, True), 3)          # (a refusal raises)
    for h, w, q in ((33, 47, 75), (64, 96, 95)):
        pin("%dx%d_q%d_mono" % (h, w, q), pillow_write(picture(h, w, 1, rng), q, None, True), 1)
    assert sum(pin_tables_of) >= 230 and len(pin_names) == 61, (sum(pin_tables_of), len(pin_names))
    pin_counts = np.concatenate(pin_counts)
    assert pin_counts.max() < 1 << 31
    # ---------------------------------------------------------------- 2: chosen counts
    chosen = O.chosen_counts()
    chosen_lengths = []
    for name, freq in chosen:
        table = O.gen_optimal_table(freq)
        assert max(O.code_lengths(*table).values(), default=0) <= 16, name
        chosen_lengths.append(table)
    # ---------------------------------------------------------------- 3: small calls
    call_names, call_layouts, call_quality, call_shapes = [], [], [], []
    call_sizes, call_blob, call_lengths, call_pillow = [], [], [], []
    stacks = {}
    for layout, sampling in O.LAYOUTS:
        c = 1 if sampling is None else 3
        for n, h, w, q in CALLS:
            key = (n, h, w, c)
            if key not in stacks:
                stacks[key] = O.stack_of(n, h, w, c, 1000 * h + w)
            frames = stacks[key]
            name = "%s_%dx%dx%d_q%d" % (layout, n, h, w, q)
            files, tables = O.encode(frames, q, sampling)
            plain = O._plain(frames, q, sampling)
            assert sum(map(len, files)) <= sum(map(len, plain)), name
            for k, (f, p) in enumerate(zip(files, plain)):
                seen = pillow_decode(f, name)
                assert seen.shape == frames[k].shape and np.array_equal(seen, pillow_decode(p, name)), (name, k)
                diff = seen.astype(np.int16) - S.ideal_decode(f).astype(np.int16)
                assert np.abs(diff).max() <= 4, (name, k)
                call_pillow.append(diff.astype(np.int8).ravel())
                call_sizes.append(len(f))
                call_blob.append(np.frombuffer(f, np.uint8))
            for t in tables:
                call_lengths.append((list(t[:16]), list(t[16:16 + int(t[:16].sum())])))
            call_names.append(name)
            call_layouts.append(layout)
            call_quality.append(q)
            call_shapes.append((n, h, w, c))
    # ---------------------------------------------------------------- 4: what libjpeg gains on the benchmark's pictures
    from PIL import ImageFile
    ImageFile.MAXBLOCK = 1 << 26                                     # (room for the optimised 1080p noise picture)
    ratio_names, ratio_bytes = [], []
    for noise in (False, True):
        for layout, sampling in O.LAYOUTS:
            frame = scene(1080, 1920, 1 if sampling is None else 3, np.random.default_rng(47 + noise), noise)
            sub = {None: None, (1, 1): 0, (2, 1): 1, (2, 2): 2}[sampling]
            ratio_names.append("%s/%s" % ("noise" if noise else "smooth", layout))
            ratio_bytes.append((len(pillow_write(frame, 90, sub, False)), len(pillow_write(frame, 90, sub, True))))
            print(ratio_names[-1], ratio_bytes[-1], round(ratio_bytes[-1][1] / ratio_bytes[-1][0], 4))
    path = os.path.join(HERE, "mjpeg_optimized_v1.npz")
    kept = {}
    for part, tables in (("pin", pin_lengths), ("chosen", chosen_lengths), ("call", call_lengths)):
        for key, value in packed_tables(tables).items():
            kept["%s_tables_%s" % (part, key)] = value
        assert np.array_equal(O.unpacked_tables(kept, part), np.stack([O.table_bytes(*t) for t in tables])), part
    np.savez_compressed(
        path, **kept, pin_names=np.array(pin_names), pin_tables_of=np.array(pin_tables_of, np.int32),
        pin_counts=pin_counts.astype(np.int32),
        chosen_names=np.array([n for n, _ in chosen]),
        call_names=np.array(call_names), call_layouts=np.array(call_layouts), call_quality=np.array(call_quality, np.int32),
        call_shapes=np.array(call_shapes, np.int32), stack_shapes=np.array(list(stacks), np.int32),
        stack_frames=np.concatenate([v.ravel() for v in stacks.values()]),
        call_sizes=np.array(call_sizes, np.int64), call_blob=np.concatenate(call_blob),
        call_pillow_diff=np.concatenate(call_pillow),
        ratio_names=np.array(ratio_names), ratio_bytes=np.array(ratio_bytes, np.int64))
    size = os.path.getsize(path)
    limit = os.path.getsize(os.path.join(HERE, "mjpeg_encode_sampled_v1.npz"))
    print("%d pinned tables of %d files, %d chosen, %d calls; %d bytes (limit %d)"
          % (sum(pin_tables_of), len(pin_names), len(chosen), len(call_names), size, limit))
    assert size <= limit


main()
