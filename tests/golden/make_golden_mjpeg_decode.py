"""Writes tests/golden/mjpeg_decode_v1.npz: the streams of the Motion-JPEG decoding tests with the pixels and status
words of the restatement (tests/jpeg_decode_checks.py, the definition of DESIGN.md §9, "Motion-JPEG decoding").

  (a) the 120 streams of mjpeg_v1.npz (their bytes stay there; here are the expected pixels, stored as the int8
      difference from Pillow's decode of the same stream in mjpeg_v1.npz, which is small and compresses well)
  (b) Pillow-written streams: 1x1, 9x17, 37x53 noise, L and RGB 4:4:4, qualities 1 / 50 / 85 / 100, each without
      restart markers, with one per MCU row, with one every 3 blocks, and with optimised Huffman tables.  The four
      variants code the same coefficients, so their pixels (asserted equal; stored as the int8 difference from
      Pillow's decode) and Pillow's decode are stored once.
  (c) hostile variants of a monochrome and a colour stream of (a); the pixels are stored as their difference modulo
      256 from the intact stream's
  (d) streams the host must refuse, each with a word the message must contain

Writing the fixture asserts the accuracy condition on (a) and (b): the clamp of the dequantiser is not active; each
component sample is within 1 of the float64 IDCT of the same dequantised coefficients, rounded and clipped; each pixel
is within 1 (monochrome) and R 3, G 3, B 4 (colour) of the ideal decode; and on (b) Pillow's decode is within the same
bounds of the ideal decode.  It asserts that (c) sets every status bit and shows the zeroed blocks.  Data only.
Run from the repository root: python tests/golden/make_golden_mjpeg_decode.py"""
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_checks as J  # noqa: E402
import jpeg_decode_checks as D  # noqa: E402

B_SHAPES = ((1, 1), (9, 17), (37, 53))
B_QUALITIES = (1, 50, 85, 100)
B_VARIANTS = (("plain", {}), ("rows", {"restart_marker_rows": 1}), ("blocks3", {"restart_marker_blocks": 3}),
              ("optimized", {"optimize": True}))
C_SOURCES = ("noise_q50_37x53x1", "noise_q90_37x53x3")
C_FLIP_SEEDS = (0, 1, 2, 3, 4, 5, 6, 7)


def hostile(data):
    """[(name, bytes)] of the hostile variants of a stream with one restart interval per MCU row"""
    data = bytes(data)
    head = D.parse_header(data)
    segs, bit = D.split_segments(data, head["scan_begin"], head["nseg"])
    assert bit == 0 and len(segs) >= 4
    out = [("cut_mid", data[:(segs[2][0] + segs[2][1]) // 2])]
    ff = data.index(b"\xff\x00", head["scan_begin"])
    out.append(("cut_ff", data[:ff + 1]))
    m1, m2 = segs[1][1], segs[2][1]                       # the markers behind segments 1 and 2
    out.append(("rst_removed", data[:m1] + data[m1 + 2:]))
    swapped = bytearray(data)
    swapped[m1 + 1], swapped[m2 + 1] = swapped[m2 + 1], swapped[m1 + 1]
    out.append(("rst_swapped", bytes(swapped)))
    for seed in C_FLIP_SEEDS:
        rng = np.random.default_rng(seed)
        at = int(rng.integers(head["scan_begin"], len(data) - 2))
        flipped = bytearray(data)
        flipped[at] ^= 1 << int(rng.integers(0, 8))
        out.append(("bitflip%d" % seed, bytes(flipped)))
    b, e = segs[2]
    out.append(("ff00", data[:b] + (b"\xff\x00" * (e - b))[:e - b] + data[e:]))
    out.append(("no_eoi", data[:-2]))
    return out


def refused(golden):
    from PIL import Image
    rng = np.random.default_rng(7)
    image = Image.fromarray(rng.integers(0, 256, (16, 24, 3), dtype=np.uint8))

    def written(**kw):
        buf = io.BytesIO()
        image.save(buf, "JPEG", quality=75, **kw)
        return buf.getvalue()
    colour = golden["bytes_noise_q90_9x17x3"].tobytes()
    sof = colour.index(b"\xff\xc0")
    twelve = bytearray(colour)
    twelve[sof + 4] = 12
    sos = colour.index(b"\xff\xda")
    scan_begin = D.parse_header(colour)["scan_begin"]
    one = b"\xff\xda" + bytes([0, 8, 1, 1, 0x00, 0, 63, 0])
    two_scans = colour[:sos] + one + colour[scan_begin:-2] + one.replace(b"\x01\x01\x00", b"\x01\x02\x11") + b"\xff\xd9"
    return [("pillow_420", written(subsampling=2), "sampling"), ("pillow_progressive", written(progressive=True,
            subsampling=0), "progressive"), ("sof_12bit", bytes(twelve), "precision"), ("two_scans", two_scans, "scan")]


def difference(pixels, pillow):
    """pixels - pillow as int8 (the two are within a few levels of each other)"""
    d = pixels.astype(np.int16) - pillow.astype(np.int16)
    assert pixels.shape == pillow.shape and np.abs(d).max() <= 8
    return d.astype(np.int8)


class Accuracy(object):
    def __init__(self):
        self.component, self.mono, self.rgb = 0, 0, np.zeros(3, int)
        self.differ = self.total = 0

    def check(self, name, data, pixels):
        head = D.parse_header(data)
        coefs, status = D.decode_coefficients(data, head)
        assert status == 0, (name, status)
        f, clamped = D.dequantised(coefs, head["qtables"])
        assert not clamped, "%s: the dequantiser's clamp is active on a valid stream" % name
        err = int(np.abs(D.integer_planes(f) - D.float_planes(f)).max())
        assert err <= 1, "%s: a component sample is %d from the float64 IDCT" % (name, err)
        self.component = max(self.component, err)
        ideal = D.ideal_decode(data, head)
        d = np.abs(pixels.astype(int) - ideal.astype(int))
        if pixels.ndim == 2:
            assert d.max() <= 1, (name, d.max())
            self.mono = max(self.mono, int(d.max()))
        else:
            worst = d.reshape(-1, 3).max(axis=0)
            assert (worst <= (3, 3, 4)).all(), (name, worst)
            self.rgb = np.maximum(self.rgb, worst)
        self.differ += int((d != 0).sum())
        self.total += d.size
        return ideal


def main():
    from PIL import Image
    golden = np.load(os.path.join(HERE, "mjpeg_v1.npz"), allow_pickle=False)
    store, acc = {}, Accuracy()
    # ------------------------------------------------------------------------------------------------ (a)
    names_a = [str(n) for n in golden["names"]]
    for name in names_a:
        data = golden["bytes_" + name].tobytes()
        pixels, status = D.decode(data)
        ideal = acc.check(name, data, pixels)
        assert status == 0 and np.array_equal(ideal, J.ideal_decode(data)), name
        store["a_dpx_" + name] = difference(pixels, golden["pillow_" + name])
    store["names_a"] = np.array(names_a)
    # ------------------------------------------------------------------------------------------------ (b)
    rng = np.random.default_rng(20261020)
    pillow_mono, pillow_rgb = 0, np.zeros(3, int)
    bases, names_b = [], []
    for h, w in B_SHAPES:
        for mode in ("L", "RGB"):
            frame = rng.integers(0, 256, (h, w) + ((3,) if mode == "RGB" else ()), dtype=np.uint8)
            for q in B_QUALITIES:
                base = "%s_q%d_%dx%d" % (mode, q, h, w)
                bases.append(base)
                first = None
                for variant, kw in B_VARIANTS:
                    buf = io.BytesIO()
                    Image.fromarray(frame).save(buf, "JPEG", quality=q, subsampling=0, **kw)
                    data = buf.getvalue()
                    name = base + "_" + variant
                    pixels, status = D.decode(data)
                    ideal = acc.check(name, data, pixels)
                    seen = np.asarray(Image.open(io.BytesIO(data)))
                    assert seen.shape == pixels.shape, name
                    if first is None:
                        first = (pixels, seen)
                        d = np.abs(seen.astype(int) - ideal.astype(int))
                        if mode == "L":
                            assert d.max() <= 1, (name, d.max())
                            pillow_mono = max(pillow_mono, int(d.max()))
                        else:
                            worst = d.reshape(-1, 3).max(axis=0)
                            assert (worst <= (3, 3, 4)).all(), (name, worst)
                            pillow_rgb = np.maximum(pillow_rgb, worst)
                    assert np.array_equal(pixels, first[0]) and np.array_equal(seen, first[1]), name
                    names_b.append(name)
                    store["b_bytes_" + name] = np.frombuffer(data, np.uint8)
                store["b_dpx_" + base] = difference(first[0], first[1])
                store["b_pillow_" + base] = first[1]
    head = D.parse_header(store["b_bytes_RGB_q85_37x53_blocks3"].tobytes())
    assert head["ri"] == 3 and head["nseg"] == 12 and (5 * 7) % 3 != 0
    assert D.parse_header(store["b_bytes_RGB_q85_37x53_plain"].tobytes())["nseg"] == 1
    assert (D.header_key(D.parse_header(store["b_bytes_RGB_q85_37x53_optimized"].tobytes()))[5]
            != D.header_key(D.parse_header(store["b_bytes_RGB_q85_37x53_plain"].tobytes()))[5])
    store["names_b"], store["bases_b"] = np.array(names_b), np.array(bases)
    # ------------------------------------------------------------------------------------------------ (c)
    names_c, status_c, bits = [], [], 0
    for source in C_SOURCES:
        for variant, data in hostile(golden["bytes_" + source]):
            name = source + "_" + variant
            head = D.parse_header(data)
            coefs, status, report = D.decode_coefficients(data, head, ret_segments=True)
            pixels, status2 = D.decode(data, head)
            assert status == status2
            bx = (head["w"] + 7) // 8
            for j, seg in enumerate(report):                 # the zeroed blocks show as sample 128
                if seg is None:
                    first = j * head["ri"]
                elif seg[0]:
                    first = seg[1]
                else:
                    continue
                last = min((j + 1) * head["ri"], bx * ((head["h"] + 7) // 8)) - 1
                # (in colour the error may sit in the MCU's Cb or Cr block, behind a Y block that decoded)
                for m in ((first, last) if head["c"] == 1 or seg is None else (last,) if last > first else ()):
                    y, x = 8 * (m // bx), 8 * (m % bx)
                    assert (pixels[y:y + 8, x:x + 8] == 128).all() and not coefs[:, m // bx, m % bx].any(), (name, j, m)
            if not variant.startswith("bitflip"):
                assert status != 0, name
            bits |= status
            names_c.append(name)
            status_c.append(status)
            store["c_bytes_" + name] = np.frombuffer(data, np.uint8)
            # modulo 256 against the intact stream's pixels: zero wherever the damage did not reach
            store["c_dpx_" + name] = pixels - (golden["pillow_" + source].astype(np.int16)
                                               + store["a_dpx_" + source]).astype(np.uint8)
    assert bits == 15, "the hostile cases set only the status bits %d" % bits
    store["names_c"], store["status_c"] = np.array(names_c), np.array(status_c, np.int32)
    # ------------------------------------------------------------------------------------------------ (d)
    names_d, words_d = [], []
    for name, data, word in refused(golden):
        try:
            D.parse_header(data)
        except ValueError as err:
            assert word in str(err), (name, err)
        else:
            raise AssertionError("%s is not refused" % name)
        names_d.append(name)
        words_d.append(word)
        store["d_bytes_" + name] = np.frombuffer(data, np.uint8)
    store["names_d"], store["words_d"] = np.array(names_d), np.array(words_d)
    store["worst_component"] = np.int64(acc.component)
    store["worst_mono"], store["worst_rgb"] = np.int64(acc.mono), acc.rgb.astype(np.int64)
    store["pixels_differ"] = np.array([acc.differ, acc.total], np.int64)
    store["pillow_worst_mono"], store["pillow_worst_rgb"] = np.int64(pillow_mono), pillow_rgb.astype(np.int64)
    path = os.path.join(HERE, "mjpeg_decode_v1.npz")
    np.savez_compressed(path, **store)
    print("%d + %d + %d + %d cases, %d bytes" % (len(names_a), len(names_b), len(names_c), len(names_d),
                                                 os.path.getsize(path)))
    print("component samples vs float64 IDCT: at most %d; pixels vs ideal decode: mono %d, RGB %s; %d of %d samples "
          "(%.2f %%) differ from the ideal decode" % (acc.component, acc.mono, acc.rgb, acc.differ, acc.total,
                                                      100.0 * acc.differ / acc.total))
    print("Pillow vs ideal decode on (b): mono %d, RGB %s" % (pillow_mono, pillow_rgb))
    print("status of (c):", dict(zip(names_c, status_c)))


if __name__ == "__main__":
    main()
