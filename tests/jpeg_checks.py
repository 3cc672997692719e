"""The Motion-JPEG stream of DESIGN.md §9, "Motion-JPEG", restated in NumPy: this file is the definition, and the
device equals it byte for byte.  Also a marker / segment parser, an AVI parser and an *ideal decode* (Huffman decode,
dequantise, float64 IDCT, round and clip, JFIF inverse matrix in float64, round and clip) that the fixture generator
holds Pillow's decoder against.  Nothing here imports the package."""
import math
import struct

import numpy as np

# ------------------------------------------------------------------------------------------------ tables
# ITU T.81 Annex K.1 / K.2, in natural (row-major) order
BASE_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
BASE_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64)

# Annex K.3 - K.6: (BITS, HUFFVAL) of the typical tables, keyed by the DHT byte Tc << 4 | Th
_AC_TAIL = [0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a,
            0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a,
            0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a]
DHT = {
    0x00: ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    0x10: ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
            0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
            0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a] + _AC_TAIL
           + [0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
              0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
              0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
              0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea,
              0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]),
    0x01: ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    0x11: ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
           [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
            0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
            0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
            0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a,
            0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a,
            0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
            0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
            0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
            0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
            0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]),
}


def _zigzag():
    order, x, y, up = [], 0, 0, True
    for _ in range(64):
        order.append(8 * y + x)
        if up:
            if x == 7:
                y, up = y + 1, False
            elif y == 0:
                x, up = x + 1, False
            else:
                x, y = x + 1, y - 1
        else:
            if y == 7:
                x, up = x + 1, True
            elif x == 0:
                y, up = y + 1, True
            else:
                x, y = x - 1, y + 1
    return np.array(order, np.int64)


ZIGZAG = _zigzag()                     # ZIGZAG[k] = natural index of the k-th coefficient in zigzag order


def quant_tables(quality):
    """(luma, chroma) in natural order, the IJG scaling of the Annex K base tables"""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError("quality is 1 .. 100, got %r" % (quality,))
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * scale + 50) // 100, 1, 255) for base in (BASE_LUMA, BASE_CHROMA))


def dct_matrix():
    """T[k][n] = rint(2**13 A[k][n]), A the orthonormal 8-point DCT-II matrix"""
    a = np.array([[(math.sqrt(1 / 8) if k == 0 else 0.5) * math.cos((2 * n + 1) * k * math.pi / 16) for n in range(8)]
                  for k in range(8)])
    return np.rint(a * 2 ** 13).astype(np.int64), a


def huffman_codes(bits, vals):
    """{symbol: (code, length)} of a (BITS, HUFFVAL) pair, Annex C"""
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return codes


def _code_arrays(key):
    code, length = np.zeros(256, np.int64), np.zeros(256, np.int64)
    for sym, (c, n) in huffman_codes(*DHT[key]).items():
        code[sym], length[sym] = c, n
    return code, length


_CODES = {key: _code_arrays(key) for key in DHT}


# ------------------------------------------------------------------------------------------------ header
def _segment(marker, payload):
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + bytes(payload)


def dht_payload(key):
    bits, vals = DHT[key]
    return bytes([key] + list(bits) + list(vals))


def header(h, w, c, quality):
    """SOI .. SOS of a frame of h x w with c = 1 or 3 components"""
    luma, chroma = quant_tables(quality)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    out += _segment(0xDB, bytes([0]) + bytes(luma[ZIGZAG].astype(np.uint8)))
    if c == 3:
        out += _segment(0xDB, bytes([1]) + bytes(chroma[ZIGZAG].astype(np.uint8)))
    comps = [(1, 0)] if c == 1 else [(1, 0), (2, 1), (3, 1)]
    out += _segment(0xC0, struct.pack(">BHHB", 8, h, w, len(comps)) + b"".join(bytes([i, 0x11, t]) for i, t in comps))
    for key in (0x00, 0x10) + ((0x01, 0x11) if c == 3 else ()):
        out += _segment(0xC4, dht_payload(key))
    out += _segment(0xDD, struct.pack(">H", (w + 7) // 8))
    out += _segment(0xDA, bytes([len(comps)]) + b"".join(bytes([i, 0x11 * t]) for i, t in comps) + bytes([0, 63, 0]))
    return out


# ------------------------------------------------------------------------------------------------ transform
def ycbcr(rgb):
    """JFIF full range in 16-bit fixed point: (h, w, 3) uint8 -> three (h, w) int64 planes"""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    return ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
            (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16,
            (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16)


def planes_of(frame):
    """the component planes of a frame, padded to multiples of 8 by repeating the last column and row"""
    frame = np.asarray(frame)
    planes = [frame.astype(np.int64)] if frame.ndim == 2 else list(ycbcr(frame))
    h, w = planes[0].shape
    return [np.pad(p, ((0, -h % 8), (0, -w % 8)), mode="edge") for p in planes]


def forward(plane, qtable):
    """(by, bx, 64) quantised coefficients in zigzag order of a padded plane (integers only)"""
    t, _ = dct_matrix()
    hh, ww = plane.shape
    x = (plane - 128).reshape(hh // 8, 8, ww // 8, 8).transpose(0, 2, 1, 3)            # [by, bx, y, n]
    rows = (np.einsum("kn,abyn->abyk", t, x) + 1024) >> 11
    s = np.einsum("vy,abyk->abvk", t, rows)                                            # coefficient * 2**15
    q = np.asarray(qtable, np.int64).reshape(8, 8)
    quant = np.sign(s) * ((np.abs(s) + (q << 14)) // (q << 15))
    return quant.reshape(hh // 8, ww // 8, 64)[:, :, ZIGZAG]


def float_quantised(plane, qtable):
    """rint(float64 DCT / Q), zigzag order: what `forward` approximates"""
    _, a = dct_matrix()
    hh, ww = plane.shape
    x = (plane - 128).astype(np.float64).reshape(hh // 8, 8, ww // 8, 8).transpose(0, 2, 1, 3)
    s = np.einsum("vy,abyn,kn->abvk", a, x, a)
    return np.rint(s / np.asarray(qtable, np.float64).reshape(8, 8)).astype(np.int64).reshape(hh // 8, ww // 8, 64)[
        :, :, ZIGZAG]


def frame_coefficients(frame, quality):
    """per component the (by, bx, 64) zigzag coefficients"""
    tables = quant_tables(quality)
    return [forward(p, tables[min(i, 1)]) for i, p in enumerate(planes_of(frame))]


# ------------------------------------------------------------------------------------------------ entropy coding
def _bit_length(v):
    v = np.abs(v)
    size = np.zeros(v.shape, np.int64)
    for k in range(12):
        size += v >= (1 << k)
    return size


def pack_bits(codes, lengths):
    """the bit strings (code, length <= 16 each) in order, padded to a byte with 1-bits: uint8 array"""
    codes, lengths = np.asarray(codes, np.int64), np.asarray(lengths, np.int64)
    shifts = lengths[:, None] - 1 - np.arange(16)[None, :]
    bits = ((codes[:, None] >> np.maximum(shifts, 0)) & 1).astype(np.uint8)[shifts >= 0]
    bits = np.concatenate([bits, np.ones(-len(bits) % 8, np.uint8)])
    return np.packbits(bits)


def stuff(data):
    """every 0xFF byte followed by 0x00"""
    data = np.asarray(data, np.uint8)
    return np.insert(data, np.flatnonzero(data == 0xFF) + 1, 0)


def segment_symbols(blocks, comp_of_block):
    """the (code, length) strings of one entropy segment.  blocks: (B, 64) zigzag coefficients in coding order,
    comp_of_block: (B,) component of each (0 = luma tables, else chroma); DC predictors start at 0"""
    blocks = np.asarray(blocks, np.int64)
    tab = np.minimum(np.asarray(comp_of_block), 1)
    dc = blocks[:, 0]
    diff = dc.copy()
    for comp in np.unique(comp_of_block):
        idx = np.flatnonzero(np.asarray(comp_of_block) == comp)
        diff[idx] = dc[idx] - np.concatenate([[0], dc[idx][:-1]])
    keys, codes, lens = [], [], []

    def emit(block, k, sub, code, length):
        keys.append((block * 65 + k) * 8 + sub)
        codes.append(code)
        lens.append(length)

    def magnitude(v, size):
        return np.where(v >= 0, v, v + (1 << size) - 1)

    dsize = _bit_length(diff)
    for t, key in ((0, 0x00), (1, 0x01)):
        sel = np.flatnonzero(tab == t)
        code, length = _CODES[key]
        emit(sel, 0, 0, code[dsize[sel]], length[dsize[sel]])
        emit(sel, 0, 1, magnitude(diff[sel], dsize[sel]), dsize[sel])
    b, k = np.nonzero(blocks[:, 1:])
    k = k + 1
    v = blocks[b, k]
    prev = np.concatenate([[0], k[:-1]])
    prev[np.concatenate([[True], b[1:] != b[:-1]])] = 0
    run = k - prev - 1
    size = _bit_length(v)
    for t, key in ((0, 0x10), (1, 0x11)):
        code, length = _CODES[key]
        sel = tab[b] == t
        bs, ks = b[sel], k[sel]
        for z in range(3):
            zs = run[sel] >= 16 * (z + 1)
            emit(bs[zs], ks[zs], z, np.full(zs.sum(), code[0xF0]), np.full(zs.sum(), length[0xF0]))
        sym = ((run[sel] & 15) << 4) | size[sel]
        emit(bs, ks, 3, code[sym], length[sym])
        emit(bs, ks, 4, magnitude(v[sel], size[sel]), size[sel])
        eob = np.flatnonzero((tab == t) & (blocks[:, 63] == 0))
        emit(eob, 64, 0, np.full(len(eob), code[0]), np.full(len(eob), length[0]))
    order = np.argsort(np.concatenate(keys), kind="stable")
    return np.concatenate(codes)[order], np.concatenate(lens)[order]


def encode_segment(blocks, comp_of_block):
    """the stuffed bytes of one entropy segment"""
    return stuff(pack_bits(*segment_symbols(blocks, comp_of_block)))


def frame_segments(frame, quality):
    """the stuffed entropy segments of a frame, one per MCU row"""
    coefs = frame_coefficients(frame, quality)
    c = len(coefs)
    by, bx = coefs[0].shape[:2]
    comp = np.tile(np.arange(c), bx)
    return [encode_segment(np.stack([co[row] for co in coefs], axis=1).reshape(bx * c, 64), comp) for row in range(by)]


def encode_frame(frame, quality=90):
    """one complete baseline JFIF file"""
    frame = np.asarray(frame)
    if frame.dtype != np.uint8 or not (frame.ndim == 2 or (frame.ndim == 3 and frame.shape[2] == 3)):
        raise ValueError("a frame is uint8 (h, w) or (h, w, 3)")
    h, w = frame.shape[:2]
    out = [header(h, w, 1 if frame.ndim == 2 else 3, quality)]
    for i, seg in enumerate(frame_segments(frame, quality)):
        if i:
            out.append(bytes([0xFF, 0xD0 + (i - 1) % 8]))
        out.append(seg.tobytes())
    out.append(b"\xff\xd9")
    return b"".join(out)


def encode(frames, quality=90):
    return [encode_frame(f, quality) for f in frames]


# ------------------------------------------------------------------------------------------------ parsing
def parse(data):
    """[(marker, payload)] of a JFIF file up to SOS, then ('scan', [segment bytes with the stuffing still in]), then
    whether EOI ends the file: (segments, scan_segments, rst_markers)"""
    data = bytes(data)
    assert data[:2] == b"\xff\xd8", "no SOI"
    segs, i = [], 2
    while True:
        assert data[i] == 0xFF, "marker expected at %d" % i
        marker, length = data[i + 1], struct.unpack(">H", data[i + 2:i + 4])[0]
        segs.append((marker, data[i + 4:i + 2 + length]))
        i += 2 + length
        if marker == 0xDA:
            break
    assert data[-2:] == b"\xff\xd9", "no EOI"
    body = np.frombuffer(data[i:-2], np.uint8)
    ff = np.flatnonzero(body[:-1] == 0xFF)
    marks = ff[(body[ff + 1] != 0)]
    assert all(0xD0 <= body[m + 1] <= 0xD7 for m in marks), "a marker other than RST inside the scan"
    scans, start = [], 0
    for m in marks:
        scans.append(body[start:m].tobytes())
        start = m + 2
    scans.append(body[start:].tobytes())
    return segs, scans, [int(body[m + 1]) for m in marks]


def _decode_tables(segs):
    tables = {}
    for marker, payload in segs:
        if marker != 0xC4:
            continue
        p = payload
        while p:
            key, bits = p[0], list(p[1:17])
            n = sum(bits)
            tables[key] = {(length, code): sym for sym, (code, length) in huffman_codes(bits, list(p[17:17 + n])).items()}
            p = p[17 + n:]
    return tables


def decode_coefficients(data):
    """(h, w, [per component (by, bx, 64) zigzag coefficients], [natural-order quantisation table per component])
    of a stream this module describes (1 x 1 sampling, a restart interval of one MCU row)"""
    segs, scans, _ = parse(data)
    qt, tables = {}, _decode_tables(segs)
    for marker, payload in segs:
        if marker == 0xDB:
            q = np.zeros(64, np.int64)
            q[ZIGZAG] = list(payload[1:65])
            qt[payload[0]] = q
        elif marker == 0xC0:
            _, h, w, nc = struct.unpack(">BHHB", payload[:6])
            tq = [payload[6 + 3 * i + 2] for i in range(nc)]
    by, bx = (h + 7) // 8, (w + 7) // 8
    assert len(scans) == by
    coefs = [np.zeros((by, bx, 64), np.int64) for _ in range(nc)]
    for row, seg in enumerate(scans):
        raw = np.frombuffer(seg, np.uint8)
        keep = np.ones(len(raw), bool)
        keep[np.flatnonzero(raw[:-1] == 0xFF) + 1] = False
        bits = np.unpackbits(raw[keep]).tolist()
        pos, pred = 0, [0] * nc

        def symbol(table):
            nonlocal pos
            code = 0
            for length in range(1, 17):
                code = (code << 1) | bits[pos]
                pos += 1
                if (length, code) in table:
                    return table[(length, code)]
            raise AssertionError("no Huffman code")

        def receive(size):
            nonlocal pos
            v = 0
            for _ in range(size):
                v = (v << 1) | bits[pos]
                pos += 1
            return v if size == 0 or v >= (1 << (size - 1)) else v - (1 << size) + 1

        for col in range(bx):
            for comp in range(nc):
                t = 0 if comp == 0 else 1
                pred[comp] += receive(symbol(tables[t]))
                block = coefs[comp][row, col]
                block[0] = pred[comp]
                k = 1
                while k < 64:
                    rs = symbol(tables[0x10 | t])
                    if rs == 0:
                        break
                    if rs == 0xF0:
                        k += 16
                        continue
                    k += rs >> 4
                    block[k] = receive(rs & 15)
                    k += 1
        assert all(bits[pos:]) and len(bits) - pos < 8, "the padding is 1-bits up to the byte"
    return h, w, coefs, [qt[t] for t in tq]


def ideal_decode(data):
    """dequantise, float64 IDCT, round and clip to 0 .. 255, JFIF inverse matrix in float64, round, clip"""
    h, w, coefs, tables = decode_coefficients(data)
    _, a = dct_matrix()
    planes = []
    for co, q in zip(coefs, tables):
        nat = np.zeros(co.shape, np.float64)
        nat[:, :, ZIGZAG] = co
        s = (nat * q).reshape(co.shape[0], co.shape[1], 8, 8)
        x = np.einsum("vy,abvk,kn->abyn", a, s, a) + 128
        plane = np.clip(np.rint(x), 0, 255).transpose(0, 2, 1, 3).reshape(co.shape[0] * 8, co.shape[1] * 8)
        planes.append(plane[:h, :w])
    if len(planes) == 1:
        return planes[0].astype(np.uint8)
    y, cb, cr = planes[0], planes[1] - 128, planes[2] - 128
    rgb = np.stack([y + 1.402 * cr, y - 0.344136 * cb - 0.714136 * cr, y + 1.772 * cb], axis=-1)
    return np.clip(np.rint(rgb), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ AVI
def parse_riff(data, start=0, end=None):
    """the chunks of a RIFF byte range: [(fourcc, offset of the data, size, list type or None)]"""
    end = len(data) if end is None else end
    out, i = [], start
    while i + 8 <= end:
        cc, size = data[i:i + 4], struct.unpack("<I", data[i + 4:i + 8])[0]
        kind = data[i + 8:i + 12] if cc in (b"RIFF", b"LIST") else None
        out.append((cc, i + 8, size, kind))
        i += 8 + size + (size & 1)
    assert i == end, "the chunks do not fill their range (%d != %d)" % (i, end)
    return out


def parse_avi(data):
    """a dict of what an AVI 1.0 file with one MJPG stream holds: avih and strh fields, the BITMAPINFOHEADER, the
    frames (offset, size) from the movi list and from idx1; asserts the structure on the way"""
    data = bytes(data)
    (cc, at, size, kind), = parse_riff(data)
    assert cc == b"RIFF" and kind == b"AVI " and size == len(data) - 8
    top = parse_riff(data, at + 4, at + size)
    assert [(c, k) for c, _, _, k in top] == [(b"LIST", b"hdrl"), (b"LIST", b"movi"), (b"idx1", None)]
    hdrl = parse_riff(data, top[0][1] + 4, top[0][1] + top[0][2])
    assert [(c, k) for c, _, _, k in hdrl] == [(b"avih", None), (b"LIST", b"strl")]
    avih = struct.unpack("<14I", data[hdrl[0][1]:hdrl[0][1] + 56])
    strl = parse_riff(data, hdrl[1][1] + 4, hdrl[1][1] + hdrl[1][2])
    assert [c for c, _, _, _ in strl] == [b"strh", b"strf"]
    strh = data[strl[0][1]:strl[0][1] + strl[0][2]]
    strf = struct.unpack("<IiiHHIIiiII", data[strl[1][1]:strl[1][1] + 40])
    movi_at = top[1][1]
    chunks = parse_riff(data, movi_at + 4, movi_at + top[1][2])
    assert all(c == b"00dc" for c, _, _, _ in chunks)
    idx = np.frombuffer(data[top[2][1]:top[2][1] + top[2][2]], np.dtype("<u4")).reshape(-1, 4)
    return {"avih": avih, "strh_type": strh[:4], "strh_handler": strh[4:8],
            "strh_scale_rate_start_length": struct.unpack("<4I", strh[20:36]), "strf": strf,
            "frames": [(o, s) for _, o, s, _ in chunks], "movi_at": movi_at, "idx": idx,
            "idx_cc": [data[top[2][1] + 16 * i:top[2][1] + 16 * i + 4] for i in range(len(idx))]}
