"""The decoder of 4:2:0 and 4:2:2 files of DESIGN.md §9, "Subsampled Motion-JPEG decoding", restated in NumPy: this
file is the definition, and the device equals it byte for byte, status words included.  Everything shared with the
1 x 1 decoder (segments, entropy decode, status bits, dequantiser, the inverse passes, the colour formula) is
jpeg_decode_checks', the header parse (parse_header(data, sampling="any")) and the MCU walk into per-component
coefficient planes included; here are libjpeg's integer triangle upsampling with its edge rules, the decode of the two
layouts through it, and a small encoder that writes such streams as inputs for tests.  Nothing here imports the package."""
import struct

import numpy as np

import jpeg_checks as J
import jpeg_decode_checks as D

LAYOUTS = ((2, 1), (2, 2))              # (H, V) of the luma component: 4:2:2, 4:2:0


# ------------------------------------------------------------------------------------------------ geometry
mcu_blocks = D.mcu_blocks               # [(component, block row in the MCU, block column in the MCU)] in coding order


def geometry(head):
    """(H, V, my, mx, ch, cw): the MCU grid and the real samples of a chroma plane"""
    hh, vv = head["sampling"]
    return hh, vv, -(-head["h"] // (8 * vv)), -(-head["w"] // (8 * hh)), -(-head["h"] // vv), -(-head["w"] // hh)


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
    head = head or D.parse_header(data, sampling="any")
    if head["c"] == 1 or tuple(head["sampling"]) == (1, 1):
        return D.decode(data, head)
    coefs, status = D.decode_coefficients(data, head)
    planes, _ = integer_planes(coefs, head["qtables"])
    return D.rgb_of(full_planes(planes, head)).astype(np.uint8), status


def ideal_decode(data, head=None):
    """dequantise, float64 IDCT, round and clip, the same integer upsampling, the JFIF inverse matrix in float64,
    round and clip"""
    head = head or D.parse_header(data, sampling="any")
    if head["c"] == 1 or tuple(head["sampling"]) == (1, 1):
        return D.ideal_decode(data, head)
    coefs, _ = D.decode_coefficients(data, head)
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
