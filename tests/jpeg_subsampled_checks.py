"""The decoder of 4:2:0 and 4:2:2 files of DESIGN.md §9, "Subsampled Motion-JPEG decoding", restated in NumPy: this
file is the definition, and the device equals it byte for byte, status words included.  Everything shared with the
1 x 1 decoder (segments, entropy decode, status bits, dequantiser, the inverse passes, the colour formula) is
jpeg_decode_checks'; here are the header parse that takes the two layouts, the MCU walk into per-component coefficient
planes, libjpeg's integer triangle upsampling with its edge rules, and a small encoder that writes such streams as
inputs for tests.  Nothing here imports the package."""
import struct

import numpy as np

import jpeg_checks as J
import jpeg_decode_checks as D

LAYOUTS = ((2, 1), (2, 2))              # (H, V) of the luma component: 4:2:2, 4:2:0


# ------------------------------------------------------------------------------------------------ header
def _walk(data):
    """[(marker, offset of the payload, payload length)] up to and including SOS, as far as the bytes allow"""
    out, i = [], 2
    while i + 4 <= len(data) and data[i] == 0xFF:
        m = data[i + 1]
        if m == 0xFF:
            i += 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            i += 2
            continue
        length = struct.unpack(">H", data[i + 2:i + 4])[0]
        if m in (0xD8, 0xD9) or length < 2 or i + 2 + length > len(data):
            break
        out.append((m, i + 4, length - 2))
        if m == 0xDA:
            break
        i += 2 + length
    return out


def parse_header(data, sampling="any"):
    """jpeg_decode_checks.parse_header with `sampling` = (H, V) of the luma component in the dict.  "1x1" refuses
    what that parser refuses; "any" also takes a 3-component frame whose luma is 2 x 1 or 2 x 2 and whose chroma
    components are 1 x 1: an MCU then covers 8H x 8V pixels, and ri and nseg count those MCUs."""
    data = bytes(data)
    if sampling == "1x1":
        return dict(D.parse_header(data), sampling=(1, 1))
    if sampling != "any":
        raise ValueError("sampling is '1x1' or 'any', got %r" % (sampling,))
    segs = _walk(data)
    sofs = [(at, n) for m, at, n in segs if m == 0xC0]
    hv = (1, 1)
    if len(sofs) == 1 and sofs[0][1] >= 15 and data[sofs[0][0]] == 8 and data[sofs[0][0] + 5] == 3:
        at = sofs[0][0] + 6
        luma, cb, cr = (data[at + 3 * k + 1] for k in range(3))
        for chroma in (cb, cr):
            if chroma != 0x11:
                raise ValueError("sampling factors %d x %d of a chroma component: only 1 x 1 chroma sampling is "
                                 "decoded" % (chroma >> 4, chroma & 15))
        if luma not in (0x11, 0x21, 0x22):
            raise ValueError("sampling factors %d x %d of the luma component: 1 x 1, 2 x 1 (4:2:2) and 2 x 2 (4:2:0) "
                             "are decoded" % (luma >> 4, luma & 15))
        hv = (luma >> 4, luma & 15)
        patched = bytearray(data)
        patched[at + 1] = 0x11
        data = bytes(patched)
    head = dict(D.parse_header(data), sampling=hv)
    if hv != (1, 1):
        ri = 0
        for m, at, n in segs:
            if m == 0xDD:
                ri = struct.unpack(">H", data[at:at + 2])[0]
        mcus = -(-head["h"] // (8 * hv[1])) * -(-head["w"] // (8 * hv[0]))
        head["ri"] = ri if ri else mcus
        head["nseg"] = -(-mcus // head["ri"])
    return head


def mcu_blocks(hv):
    """the blocks of an MCU in coding order: [(component, block row in the MCU, block column in the MCU)]"""
    return [(0, v, u) for v in range(hv[1]) for u in range(hv[0])] + [(1, 0, 0), (2, 0, 0)]


def geometry(head):
    """(H, V, my, mx, ch, cw): the MCU grid and the real samples of a chroma plane"""
    hh, vv = head["sampling"]
    return hh, vv, -(-head["h"] // (8 * vv)), -(-head["w"] // (8 * hh)), -(-head["h"] // vv), -(-head["w"] // hh)


def header_key(head):
    """what two frames must share to go into one call"""
    return D.header_key(head) + (tuple(head["sampling"]),)


# ------------------------------------------------------------------------------------------------ entropy decode
def decode_coefficients(data, head=None, ret_segments=False):
    """([Y (my * V, mx * H, 64), Cb (my, mx, 64), Cr (my, mx, 64)] int64 quantised coefficients in natural order, the
    status word).  After an error the block where it happened and every later block of the segment are zero; earlier
    blocks of the same MCU keep their coefficients.  ret_segments: also per segment None (missing) or (status bit or
    0, the MCU of the error or None, the index of the block in that MCU or None)"""
    data = bytes(data)
    head = head or parse_header(data)
    hh, vv, my, mx, _, _ = geometry(head)
    ri = head["ri"]
    segs, status = D.split_segments(data, head["scan_begin"], head["nseg"])
    luts = [(D._lut(dc), D._lut(ac)) for dc, ac in head["huff"]]
    coefs = [np.zeros((my * vv, mx * hh, 64), np.int64), np.zeros((my, mx, 64), np.int64),
             np.zeros((my, mx, 64), np.int64)]
    walk, report = mcu_blocks((hh, vv)), []
    for j, seg in enumerate(segs):
        report.append(None if seg is None else (0, None, None))
        if seg is None:
            continue
        bits, pred = D._Bits(D.unstuffed(data, *seg)), [0, 0, 0]
        dead = False
        for m in range(j * ri, min((j + 1) * ri, my * mx)):
            row, col = m // mx, m % mx
            for k, (comp, v, u) in enumerate(walk):
                st, block, pred[comp] = D.decode_block(bits, luts[comp][0], luts[comp][1], pred[comp])
                if st:
                    status |= st
                    dead = True
                    report[-1] = (st, m, k)
                    break
                if comp == 0:
                    coefs[0][row * vv + v, col * hh + u] = block
                else:
                    coefs[comp][row, col] = block
            if dead:
                break
    return (coefs, status, report) if ret_segments else (coefs, status)


# ------------------------------------------------------------------------------------------------ reconstruction
def _planes(coefs, qtables, inverse):
    out, clamped = [], False
    for k, co in enumerate(coefs):
        f, cl = D.dequantised(co[None], np.asarray(qtables)[k:k + 1])
        out.append(inverse(f)[0])
        clamped = clamped or cl
    return out, clamped


def integer_planes(coefs, qtables):
    """([Y, Cb, Cr] padded sample planes of the pinned inverse transform, whether the dequantiser's clamp was active)"""
    return _planes(coefs, qtables, D.integer_planes)


def float_planes(coefs, qtables):
    """the same from the float64 IDCT, rounded and clipped"""
    return _planes(coefs, qtables, D.float_planes)


def upsample(plane, hv, h, w):
    """libjpeg's triangle filter in integers: a chroma plane with at least ceil(h / V) x ceil(w / H) real samples ->
    (h, w).  Samples outside the real ones are the nearest real sample; with at most 2 real columns every sample is
    replicated in both directions."""
    hh, vv = hv
    chh, cw = -(-h // vv), -(-w // hh)
    c = np.asarray(plane, np.int64)[:chh, :cw]
    if cw <= 2:
        return np.repeat(np.repeat(c, vv, axis=0), hh, axis=1)[:h, :w]
    if vv == 2:
        up = np.pad(c, ((1, 1), (0, 0)), mode="edge")
        s = np.empty((2 * chh, cw), np.int64)
        s[0::2] = 3 * c + up[:-2]
        s[1::2] = 3 * c + up[2:]
        bias, shift = (8, 7), 4
    else:
        s, bias, shift = c, (1, 2), 2
    side = np.pad(s, ((0, 0), (1, 1)), mode="edge")
    out = np.empty((s.shape[0], 2 * cw), np.int64)
    out[:, 0::2] = (3 * s + side[:, :-2] + bias[0]) >> shift
    out[:, 1::2] = (3 * s + side[:, 2:] + bias[1]) >> shift
    return out[:h, :w]


def full_planes(planes, head):
    """(3, h, w): Y cropped, Cb and Cr upsampled"""
    h, w, hv = head["h"], head["w"], head["sampling"]
    return np.stack([planes[0][:h, :w], upsample(planes[1], hv, h, w), upsample(planes[2], hv, h, w)])


def decode(data, head=None):
    """(the frame, uint8 (h, w, 3) RGB or (h, w); the status word) of one stored file"""
    head = head or parse_header(data)
    if head["c"] == 1 or tuple(head["sampling"]) == (1, 1):
        return D.decode(data, head)
    coefs, status = decode_coefficients(data, head)
    planes, _ = integer_planes(coefs, head["qtables"])
    return D.rgb_of(full_planes(planes, head)).astype(np.uint8), status


def ideal_decode(data, head=None):
    """dequantise, float64 IDCT, round and clip, the same integer upsampling, the JFIF inverse matrix in float64,
    round and clip"""
    head = head or parse_header(data)
    if head["c"] == 1 or tuple(head["sampling"]) == (1, 1):
        return D.ideal_decode(data, head)
    coefs, _ = decode_coefficients(data, head)
    planes, _ = float_planes(coefs, head["qtables"])
    return D.ideal_rgb_of(full_planes(planes, head)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ an encoder
def encode_frame(frame, quality=90, sampling=(2, 2), ri=None):
    """one baseline JFIF file of an (h, w, 3) uint8 frame with luma sampling (H, V) = (2, 1) or (2, 2): test input,
    not a pinned format.  The chroma planes are box averages ((sum + H V / 2) // (H V)) of the planes padded by
    repeating the edge; the coefficients are jpeg_checks.forward's, the entropy code jpeg_checks.encode_segment's
    with the Annex K tables.  ri: MCUs per restart interval (None: one MCU row; 0: no DRI and no restart marker)."""
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3 and tuple(sampling) in LAYOUTS
    hh, vv = sampling
    h, w = frame.shape[:2]
    my, mx = -(-h // (8 * vv)), -(-w // (8 * hh))
    y, cb, cr = J.ycbcr(frame)
    pad = lambda p, rows, cols: np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")

    def box(p):
        p = pad(p, -(-h // vv) * vv, -(-w // hh) * hh)
        total = p.reshape(p.shape[0] // vv, vv, p.shape[1] // hh, hh).sum(axis=(1, 3))
        return pad((total + hh * vv // 2) // (hh * vv), 8 * my, 8 * mx)
    luma, chroma = J.quant_tables(quality)
    cy = J.forward(pad(y, 8 * vv * my, 8 * hh * mx), luma)
    cc = [J.forward(box(p), chroma) for p in (cb, cr)]
    blocks = np.empty((my * mx, hh * vv + 2, 64), np.int64)
    walk = mcu_blocks(sampling)
    rows, cols = np.divmod(np.arange(my * mx), mx)
    for k, (comp, v, u) in enumerate(walk):
        blocks[:, k] = cy[rows * vv + v, cols * hh + u] if comp == 0 else cc[comp - 1][rows, cols]
    comp = np.array([c for c, _, _ in walk])
    ri = mx if ri is None else ri
    head = bytearray(J.header(h, w, 3, quality))
    assert head[-20:-16] == b"\xff\xdd\x00\x04" and head[-14:-12] == b"\xff\xda"
    sof = bytes(head).index(b"\xff\xc0\x00\x11\x08")
    assert head[sof + 11] == 0x11
    head[sof + 11] = hh << 4 | vv
    out = [bytes(head[:-20]), J._segment(0xDD, struct.pack(">H", ri)) if ri else b"", bytes(head[-14:])]
    step = ri if ri else my * mx
    for i, m0 in enumerate(range(0, my * mx, step)):
        if i:
            out.append(bytes([0xFF, 0xD0 + (i - 1) % 8]))
        part = blocks[m0:m0 + step]
        out.append(J.encode_segment(part.reshape(-1, 64), np.tile(comp, len(part))).tobytes())
    out.append(b"\xff\xd9")
    return b"".join(out)


# ------------------------------------------------------------------------------------------------ the fixture
def fixture_cases(path):
    """tests/golden/mjpeg_subsampled_v1.npz as {'a' | 'b': [(name, bytes, expected pixels, expected status)],
    'c': [(name, bytes, the word its refusal must hold)]}.  (a) stores the pixels per picture as the int8 difference
    from Pillow's decode, (b) as the difference modulo 256 from the pixels of the intact stream it was made from."""
    z = np.load(path, allow_pickle=False)

    def streams(kind):
        blob, offsets = z[kind + "_blob"], z[kind + "_offsets"]
        return [blob[offsets[k]:offsets[k + 1]].tobytes() for k in range(len(offsets) - 1)]
    pixels, at = {}, 0
    for base, (h, w) in zip(z["bases_a"], z["a_shapes"]):
        n = int(h) * int(w) * 3
        pixels[str(base)] = (z["a_pillow"][at:at + n].astype(np.int16) + z["a_dpx"][at:at + n]).astype(np.uint8).reshape(
            int(h), int(w), 3)
        at += n
    out = {"a": [(str(name), data, pixels[str(name).rsplit("_", 1)[0]], 0)
                 for name, data in zip(z["names_a"], streams("a"))], "b": [], "c": []}
    intact = {name: want for name, _, want, _ in out["a"]}
    at = 0
    for name, data, status in zip(z["names_b"], streams("b"), z["status_b"]):
        source = [s for s in intact if str(name).startswith(s + "_")][0]
        n = intact[source].size
        out["b"].append((str(name), data, intact[source] + z["b_dpx"][at:at + n].reshape(intact[source].shape), int(status)))
        at += n
    out["c"] = [(str(name), data, str(word)) for name, data, word in zip(z["names_c"], streams("c"), z["words_c"])]
    return out, z
