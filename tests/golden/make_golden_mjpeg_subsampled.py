"""Writes tests/golden/mjpeg_subsampled_v1.npz: 4:2:0 and 4:2:2 streams with the pixels and status words of the
restatement (tests/jpeg_subsampled_checks.py, the definition of DESIGN.md §9, "Subsampled Motion-JPEG decoding").

  (a) Pillow-written RGB noise in both layouts, h x w of 1x1, 5x3 (two chroma columns: replication), 3x5 (three: the
      smallest triangle), 16x16 (one 4:2:0 MCU), 17x33 (a row and a column beyond an MCU) and 37x53, qualities 1 / 50 /
      85 / 100, each without restart markers, with one per MCU row, with one every 3 MCUs and with optimised Huffman
      tables; one smooth picture per layout.  The four variants code the same coefficients, so their pixels (asserted
      equal; stored as the int8 difference from Pillow's decode) and Pillow's decode are stored once.
  (b) hostile variants of the 37x53 quality-50 stream with row restarts of each layout; the pixels are stored as their
      difference modulo 256 from the intact stream's.  `cut_in_mcu` ends the file inside an MCU behind its first
      block: the MCU's earlier blocks keep their coefficients.
  (c) streams that sampling="any" still refuses (the SOF bytes of a 4:2:0 stream patched), each with a word the
      message must contain

The streams of a group lie in one array one behind the other (they share most of their bytes, which compresses).

Writing the fixture asserts the accuracy condition on (a): the clamp of the dequantiser is not active; each upsampled
component sample is within 1 of the same integer upsampling of the float64 IDCT's planes, rounded and clipped; each
pixel is within R 3, G 3, B 4 of the float64 colour matrix on those planes.  The distances to Pillow's own decode
(libjpeg's), RGB and YCbCr, are measurements; their maxima are recorded.  Data only.
Run from the repository root: python tests/golden/make_golden_mjpeg_subsampled.py"""
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_decode_checks as D  # noqa: E402
import jpeg_subsampled_checks as S  # noqa: E402

LAYOUTS = (("420", 2, (2, 2)), ("422", 1, (2, 1)))          # name, Pillow's subsampling, (H, V)
A_SHAPES = ((1, 1), (5, 3), (3, 5), (16, 16), (17, 33), (37, 53))
A_QUALITIES = (1, 50, 85, 100)
A_VARIANTS = (("plain", {}), ("rows", {"restart_marker_rows": 1}), ("blocks3", {"restart_marker_blocks": 3}),
              ("optimized", {"optimize": True}))
B_SOURCE = "q50_37x53"
FLIP_SEEDS = (0, 1, 2, 3, 4, 5, 6, 7)
REFUSED = (("luma_1x2", 0, 0x12, "sampling"), ("luma_4x1", 0, 0x41, "sampling"), ("cb_2x1", 1, 0x21, "sampling"))


def written(frame, quality, subsampling, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, "JPEG", quality=quality, subsampling=subsampling, **kw)
    return buf.getvalue()


def pillow_decodes(data):
    """(Pillow's RGB decode, its YCbCr output with the chroma upsampled by libjpeg)"""
    from PIL import Image
    rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    image = Image.open(io.BytesIO(data))
    image.draft("YCbCr", image.size)
    assert image.mode == "YCbCr"
    return rgb, np.asarray(image)


def hostile(data):
    """[(name, bytes)] of the hostile variants of a stream with one restart interval per MCU row: the family of
    make_golden_mjpeg_decode.py's (c), on the first three segments"""
    data = bytes(data)
    head = D.parse_header(data, sampling="any")
    segs, bit = D.split_segments(data, head["scan_begin"], head["nseg"])
    assert bit == 0 and len(segs) >= 3
    out = [("cut_mid", data[:(segs[1][0] + segs[1][1]) // 2])]
    ff = data.index(b"\xff\x00", head["scan_begin"])
    out.append(("cut_ff", data[:ff + 1]))
    m0, m1 = segs[0][1], segs[1][1]                       # the markers behind segments 0 and 1
    out.append(("rst_removed", data[:m0] + data[m0 + 2:]))
    swapped = bytearray(data)
    swapped[m0 + 1], swapped[m1 + 1] = swapped[m1 + 1], swapped[m0 + 1]
    out.append(("rst_swapped", bytes(swapped)))
    for seed in FLIP_SEEDS:
        rng = np.random.default_rng(seed)
        at = int(rng.integers(head["scan_begin"], len(data) - 2))
        flipped = bytearray(data)
        flipped[at] ^= 1 << int(rng.integers(0, 8))
        out.append(("bitflip%d" % seed, bytes(flipped)))
    b, e = segs[1]
    out.append(("ff00", data[:b] + (b"\xff\x00" * (e - b))[:e - b] + data[e:]))
    out.append(("no_eoi", data[:-2]))
    return out


def cut_in_mcu(data):
    """the stream cut at the first byte of its third segment where the error falls behind the first block of an MCU"""
    head = D.parse_header(data, sampling="any")
    segs, _ = D.split_segments(data, head["scan_begin"], head["nseg"])
    for cut in range(segs[2][0] + 1, segs[2][1]):
        coefs, status, report = D.decode_coefficients(data[:cut], head, ret_segments=True)
        if report[2] and report[2][0] and report[2][2] >= 1:
            return data[:cut]
    raise AssertionError("no cut of segment 2 ends inside an MCU")


def check_kept_blocks(name, data):
    """an error at block k of MCU m zeroes block k and what follows; the blocks 0 .. k - 1 of m stay: whether one
    case shows kept coefficients"""
    head = D.parse_header(data, sampling="any")
    hh, vv, my, mx, _, _ = S.geometry(head)
    coefs, status, report = D.decode_coefficients(data, head, ret_segments=True)
    walk, shown = S.mcu_blocks((hh, vv)), False
    for j, seg in enumerate(report):
        if not seg or not seg[0]:
            continue
        _, m, k = seg
        last = min((j + 1) * head["ri"], my * mx)
        for mm in range(m, last):
            for kk, (comp, v, u) in enumerate(walk):
                block = coefs[0][(mm // mx) * vv + v, (mm % mx) * hh + u] if comp == 0 else coefs[comp][mm // mx, mm % mx]
                if (mm, kk) >= (m, k):
                    assert not block.any(), (name, j, mm, kk)
                elif block.any():
                    shown = True
    return shown


def main():
    store = {}
    rng = np.random.default_rng(20261019)
    worst_component, worst_rgb, differ, total = 0, np.zeros(3, int), 0, 0
    pillow_rgb, pillow_ycc = np.zeros(3, int), np.zeros(3, int)
    # ------------------------------------------------------------------------------------------------ (a)
    names_a, bases_a, streams_a, shapes_a, pillow_a, dpx_a = [], [], [], [], [], []
    yy, xx = np.mgrid[:37, :53]
    smooth = np.stack([4 * xx + yy, 255 - 3 * yy - xx, 2 * (xx + yy)], axis=-1).clip(0, 255).astype(np.uint8)
    for layout, subsampling, hv in LAYOUTS:
        pictures = [("%s_q%d_%dx%d" % (layout, q, h, w), frame, q)
                    for h, w in A_SHAPES for frame in [rng.integers(0, 256, (h, w, 3), dtype=np.uint8)]
                    for q in A_QUALITIES] + [("%s_smooth_q85_37x53" % layout, smooth, 85)]
        for base, frame, q in pictures:
            first = None
            for variant, kw in A_VARIANTS:
                name = base + "_" + variant
                data = written(frame, q, subsampling, **kw)
                head = D.parse_header(data, sampling="any")
                assert head["sampling"] == hv and head["c"] == 3, name
                coefs, status = D.decode_coefficients(data, head)
                planes, clamped = S.integer_planes(coefs, head["qtables"])
                ideal_planes, _ = S.float_planes(coefs, head["qtables"])
                assert status == 0 and not clamped, name
                full, ideal_full = S.full_planes(planes, head), S.full_planes(ideal_planes, head)
                err = int(np.abs(full - ideal_full).max())
                assert err <= 1, "%s: an upsampled component sample is %d from the ideal one" % (name, err)
                worst_component = max(worst_component, err)
                pixels, _ = S.decode(data, head)
                d = np.abs(pixels.astype(int) - S.ideal_decode(data, head).astype(int))
                worst = d.reshape(-1, 3).max(axis=0)
                assert (worst <= (3, 3, 4)).all(), (name, worst)
                worst_rgb = np.maximum(worst_rgb, worst)
                differ, total = differ + int((d != 0).sum()), total + d.size
                seen, seen_ycc = pillow_decodes(data)
                if first is None:
                    first = (pixels, seen)
                    pillow_rgb = np.maximum(pillow_rgb, np.abs(pixels.astype(int) - seen).reshape(-1, 3).max(axis=0))
                    pillow_ycc = np.maximum(pillow_ycc, np.abs(full.transpose(1, 2, 0) - seen_ycc)
                                            .reshape(-1, 3).max(axis=0))
                assert np.array_equal(pixels, first[0]) and np.array_equal(seen, first[1]), name
                names_a.append(name)
                streams_a.append(data)
            d = first[0].astype(np.int16) - first[1].astype(np.int16)
            assert np.abs(d).max() <= 8, base
            bases_a.append(base)
            shapes_a.append(frame.shape[:2])
            pillow_a.append(first[1].ravel())
            dpx_a.append(d.astype(np.int8).ravel())
    by_name = dict(zip(names_a, streams_a))
    head = D.parse_header(by_name["420_q85_37x53_blocks3"], sampling="any")
    assert head["ri"] == 3 and head["nseg"] == 4 and (3 * 4) % 3 == 0
    head = D.parse_header(by_name["422_q85_37x53_blocks3"], sampling="any")
    assert head["ri"] == 3 and head["nseg"] == 7 and (5 * 4) % 3 != 0
    assert D.parse_header(by_name["420_q85_37x53_plain"], sampling="any")["nseg"] == 1
    assert D.parse_header(by_name["420_q85_37x53_rows"], sampling="any")["nseg"] == 3
    assert (D.header_key(D.parse_header(by_name["420_q85_37x53_optimized"], sampling="any"))[5]
            != D.header_key(D.parse_header(by_name["420_q85_37x53_plain"], sampling="any"))[5])
    store["names_a"], store["bases_a"] = np.array(names_a), np.array(bases_a)
    store["a_blob"] = np.frombuffer(b"".join(streams_a), np.uint8)
    store["a_offsets"] = np.concatenate([[0], np.cumsum([len(s) for s in streams_a])]).astype(np.int64)
    store["a_shapes"] = np.array(shapes_a, np.int64)
    store["a_pillow"], store["a_dpx"] = np.concatenate(pillow_a), np.concatenate(dpx_a)
    # ------------------------------------------------------------------------------------------------ (b)
    names_b, status_b, streams_b, dpx_b, bits, kept = [], [], [], [], 0, 0
    for layout, _, _ in LAYOUTS:
        source = "%s_%s_rows" % (layout, B_SOURCE)
        intact, _ = S.decode(by_name[source])
        for variant, data in hostile(by_name[source]) + [("cut_in_mcu", cut_in_mcu(by_name[source]))]:
            name = source + "_" + variant
            head = D.parse_header(data, sampling="any")
            pixels, status = S.decode(data, head)
            assert status == D.decode_coefficients(data, head)[1]
            shown = check_kept_blocks(name, data)
            kept += shown
            assert shown or variant != "cut_in_mcu", name
            if not variant.startswith("bitflip"):
                assert status != 0, name
            bits |= status
            names_b.append(name)
            status_b.append(status)
            streams_b.append(data)
            dpx_b.append((pixels - intact).ravel())             # modulo 256: zero where the damage did not reach
    assert bits == 15, "the hostile cases set only the status bits %d" % bits
    store["names_b"], store["status_b"] = np.array(names_b), np.array(status_b, np.int32)
    store["b_blob"] = np.frombuffer(b"".join(streams_b), np.uint8)
    store["b_offsets"] = np.concatenate([[0], np.cumsum([len(s) for s in streams_b])]).astype(np.int64)
    store["b_dpx"] = np.concatenate(dpx_b)
    # ------------------------------------------------------------------------------------------------ (c)
    good = by_name["420_q85_17x33_plain"]
    sof = good.index(b"\xff\xc0\x00\x11\x08")
    streams_c = []
    for name, comp, factors, word in REFUSED:
        bad = bytearray(good)
        bad[sof + 11 + 3 * comp] = factors
        try:
            D.parse_header(bytes(bad), sampling="any")
        except ValueError as err:
            assert word in str(err), (name, err)
        else:
            raise AssertionError("%s is not refused" % name)
        streams_c.append(bytes(bad))
    store["names_c"], store["words_c"] = np.array([r[0] for r in REFUSED]), np.array([r[3] for r in REFUSED])
    store["c_blob"] = np.frombuffer(b"".join(streams_c), np.uint8)
    store["c_offsets"] = np.concatenate([[0], np.cumsum([len(s) for s in streams_c])]).astype(np.int64)
    store["worst_component"], store["worst_rgb"] = np.int64(worst_component), worst_rgb.astype(np.int64)
    store["pixels_differ"] = np.array([differ, total], np.int64)
    store["pillow_worst_rgb"], store["pillow_worst_ycc"] = pillow_rgb.astype(np.int64), pillow_ycc.astype(np.int64)
    path = os.path.join(HERE, "mjpeg_subsampled_v1.npz")
    np.savez_compressed(path, **store)
    print("%d + %d + %d cases, %d bytes" % (len(names_a), len(names_b), len(REFUSED), os.path.getsize(path)))
    print("upsampled component samples vs the ideal ones: at most %d; pixels vs ideal decode: RGB %s; %d of %d samples "
          "(%.2f %%) differ from the ideal decode" % (worst_component, worst_rgb, differ, total, 100.0 * differ / total))
    print("restatement vs Pillow: RGB %s, YCbCr %s; %d hostile cases show kept blocks" % (pillow_rgb, pillow_ycc, kept))
    print("status of (b):", dict(zip(names_b, status_b)))


if __name__ == "__main__":
    main()
