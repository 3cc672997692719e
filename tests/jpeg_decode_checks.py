"""The Motion-JPEG decoder of DESIGN.md §9, "Motion-JPEG decoding", restated in NumPy: this file is the definition,
and the device equals it byte for byte, status words included.  The header parse of every sampling layout with its
refusals, the segment splitter, the entropy decode over the MCUs of every layout with its status bits, the integer
dequantiser and inverse transform, the fixed-point colour conversion (what only 4:2:0 and 4:2:2 files need is
jpeg_subsampled_checks.py); also the float64 decode of the same coefficients that the accuracy condition is stated against.
Nothing here imports the package."""
import os
import shutil
import struct
import subprocess

import numpy as np

import jpeg_checks as J

BAD_CODE, OVERRUN, TRUNCATED, MARKER = 1, 2, 4, 8
SHIFT1, SHIFT2 = 9, 17

_SOF_NAMES = {0xC1: "extended sequential", 0xC2: "progressive", 0xC3: "lossless", 0xC5: "differential sequential",
              0xC6: "differential progressive", 0xC7: "differential lossless", 0xC9: "arithmetic sequential",
              0xCA: "arithmetic progressive", 0xCB: "arithmetic lossless", 0xCD: "arithmetic differential",
              0xCE: "arithmetic differential progressive", 0xCF: "arithmetic differential lossless"}


# ------------------------------------------------------------------------------------------------ header
def parse_header(data, sampling="1x1"):
    """what a stored file's header says, or ValueError naming what the decoder does not take: dict of h, w, c,
    sampling (H, V) of the luma component, ri (the restart interval in MCUs of 8H x 8V pixels; the MCUs of the frame
    where DRI is absent or 0), nseg, scan_begin, qtables (c, 64) uint8 in natural order, huff: per component ((BITS,
    HUFFVAL) of its DC table, of its AC table).  sampling="1x1" takes 1 component (of any factors, decoded as 1 x 1)
    or 3 of 1 x 1; "any" also takes 3 components whose luma is 2 x 1 (4:2:2) or 2 x 2 (4:2:0) and whose chroma
    components are 1 x 1 ("Subsampled Motion-JPEG decoding")."""
    if sampling not in ("1x1", "any"):
        raise ValueError("sampling is '1x1' or 'any', got %r" % (sampling,))
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise ValueError("no SOI at the start")
    i, qt, huff, sof, ri = 2, {}, {}, None, 0
    while True:
        if i + 4 > len(data):
            raise ValueError("the file ends before SOS")
        if data[i] != 0xFF:
            raise ValueError("a marker is expected at byte %d, found %02x" % (i, data[i]))
        m = data[i + 1]
        if m == 0xFF:
            i += 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            i += 2
            continue
        if m in (0xD8, 0xD9):
            raise ValueError("marker %02x before SOS" % m)
        length = struct.unpack(">H", data[i + 2:i + 4])[0]
        if length < 2 or i + 2 + length > len(data):
            raise ValueError("the segment of marker %02x at byte %d leaves the file" % (m, i))
        p = data[i + 4:i + 2 + length]
        if m == 0xDB:
            while p:
                if p[0] >> 4:
                    raise ValueError("a 16-bit quantisation table")
                if len(p) < 65 or (p[0] & 15) > 3:
                    raise ValueError("a damaged DQT segment")
                table = np.zeros(64, np.uint8)
                table[J.ZIGZAG] = list(p[1:65])
                qt[p[0] & 15], p = table, p[65:]
        elif m == 0xC4:
            while p:
                if len(p) < 17:
                    raise ValueError("a damaged DHT segment")
                bits = list(p[1:17])
                n = sum(bits)
                if (p[0] >> 4) > 1 or (p[0] & 15) > 3 or n > 256 or len(p) < 17 + n:
                    raise ValueError("a damaged DHT segment")
                code = 0
                for length_ in range(1, 17):
                    code += bits[length_ - 1]
                    if code > (1 << length_):
                        raise ValueError("a DHT segment with more codes of %d bits than there are" % length_)
                    code <<= 1
                huff[p[0]], p = (bits, list(p[17:17 + n])), p[17 + n:]
        elif m in _SOF_NAMES or m == 0xC0:
            if len(p) < 6:
                raise ValueError("a damaged frame header")
            precision, h, w, nc = struct.unpack(">BHHB", p[:6])
            if precision != 8:
                raise ValueError("sample precision %d: only 8-bit precision is decoded" % precision)
            if m != 0xC0:
                raise ValueError("%s mode (SOF%d): only baseline sequential is decoded" % (_SOF_NAMES[m], m - 0xC0))
            if sof is not None:
                raise ValueError("two frame headers")
            if nc not in (1, 3) or len(p) < 6 + 3 * nc:
                raise ValueError("%d components: 1 or 3 are decoded" % nc)
            comps = [(p[6 + 3 * k], p[7 + 3 * k], p[8 + 3 * k]) for k in range(nc)]
            luma = (1, 1)
            for k, (cid, hv, tq) in enumerate(comps):
                if hv == 0x11 or nc == 1:
                    continue
                if sampling == "1x1":
                    raise ValueError("sampling factors %d x %d (chroma subsampling such as 4:2:0 or 4:2:2): only 1 x 1 "
                                     "sampling is decoded" % (hv >> 4, hv & 15))
                if k:
                    raise ValueError("sampling factors %d x %d of a chroma component: only 1 x 1 chroma sampling is "
                                     "decoded" % (hv >> 4, hv & 15))
                if hv not in (0x21, 0x22):
                    raise ValueError("sampling factors %d x %d of the luma component: 1 x 1, 2 x 1 (4:2:2) and 2 x 2 (4:2:0) "
                                     "are decoded" % (hv >> 4, hv & 15))
                luma = (hv >> 4, hv & 15)
            if h == 0:
                raise ValueError("a frame height of 0 (DNL) is not decoded")
            if w == 0:
                raise ValueError("a frame width of 0")
            sof = (h, w, comps, luma)
        elif m == 0xCC:
            raise ValueError("arithmetic coding (DAC) is not decoded")
        elif m == 0xDC:
            raise ValueError("DNL is not decoded")
        elif m == 0xDD:
            if len(p) < 2:
                raise ValueError("a damaged DRI segment")
            ri = struct.unpack(">H", p[:2])[0]
        elif m == 0xDA:
            if sof is None:
                raise ValueError("SOS before the frame header")
            h, w, comps, luma = sof
            ns = p[0] if p else 0
            if len(p) < 1 + 2 * ns + 3:
                raise ValueError("a damaged scan header")
            if ns != len(comps) or [p[1 + 2 * k] for k in range(ns)] != [cid for cid, _, _ in comps]:
                raise ValueError("more than one scan: this scan holds %d of the %d components" % (ns, len(comps)))
            if (p[1 + 2 * ns], p[2 + 2 * ns], p[3 + 2 * ns]) != (0, 63, 0):
                raise ValueError("a scan with Ss %d, Se %d, Ah/Al %02x is not baseline sequential"
                                 % (p[1 + 2 * ns], p[2 + 2 * ns], p[3 + 2 * ns]))
            tables = []
            for k, (cid, _, tq) in enumerate(comps):
                td, ta = p[2 + 2 * k] >> 4, p[2 + 2 * k] & 15
                if tq not in qt:
                    raise ValueError("quantisation table %d is not defined" % tq)
                if td not in huff or (0x10 | ta) not in huff:
                    raise ValueError("Huffman table %d / %d is not defined" % (td, ta))
                tables.append((huff[td], huff[0x10 | ta]))
            mcus = -(-h // (8 * luma[1])) * -(-w // (8 * luma[0]))
            ri = ri if ri else mcus
            return dict(h=h, w=w, c=len(comps), sampling=luma, ri=ri, nseg=(mcus + ri - 1) // ri,
                        scan_begin=i + 2 + length, qtables=np.stack([qt[tq] for _, _, tq in comps]), huff=tables)
        i += 2 + length


# ------------------------------------------------------------------------------------------------ segments
def split_segments(data, scan_begin, nseg):
    """the entropy segments of a file whose scan data begins at scan_begin: ([(begin, end) or None] * nseg, the
    marker-sequence bit).  The data is split at every FF xx with xx not 00 or FF; the k-th such marker ends segment
    k and, when it is RST(k mod 8), begins segment k + 1; the first other one ends the scan.  Without one the last
    segment ends with the file."""
    b = np.frombuffer(bytes(data), np.uint8)
    begin = min(max(int(scan_begin), 0), len(b))
    marks = np.flatnonzero((b[:-1] == 0xFF) & (b[1:] != 0) & (b[1:] != 0xFF)) if len(b) > 1 else np.zeros(0, np.int64)
    segs, term = [], None
    for k, m in enumerate(int(m) for m in marks[marks >= begin]):
        segs.append((begin, m))
        if b[m + 1] != 0xD0 + k % 8:
            term = int(b[m + 1])
            break
        begin = m + 2
    else:
        segs.append((begin, len(b)))
    bad = term != 0xD9 or len(segs) != nseg
    return (segs + [None] * nseg)[:nseg], MARKER if bad else 0


def unstuffed(data, begin, end):
    """the bytes of a segment: FF 00 inside it is the byte FF, every other byte is itself"""
    raw = np.frombuffer(bytes(data[begin:end]), np.uint8)
    keep = np.ones(len(raw), bool)
    ff = np.flatnonzero(raw[:-1] == 0xFF) if len(raw) > 1 else np.zeros(0, np.int64)
    keep[ff[raw[ff + 1] == 0] + 1] = False
    return raw[keep].tobytes()


# ------------------------------------------------------------------------------------------------ entropy decode
_LUTS = {}


def _lut(table):
    """[the next 16 bits] -> length << 8 | symbol of the code that begins them, 0 where none does"""
    bits, vals = table
    key = (tuple(bits), tuple(vals))
    if key not in _LUTS:
        lut = np.zeros(65536, np.int64)
        for sym, (code, length) in J.huffman_codes(bits, vals).items():
            lut[code << (16 - length):(code + 1) << (16 - length)] = length << 8 | sym
        _LUTS[key] = lut.tolist()
    return _LUTS[key]


class _Bits(object):
    def __init__(self, raw):
        self.raw, self.pos, self.nbits = raw + b"\0\0\0", 0, 8 * len(raw)

    def peek16(self):
        """the next 16 bits, zeros behind the end"""
        i, raw = self.pos >> 3, self.raw
        return ((raw[i] << 16 | raw[i + 1] << 8 | raw[i + 2]) >> (8 - (self.pos & 7))) & 0xFFFF if i < len(raw) - 3 else 0

    def symbol(self, lut):
        """(status, length, symbol) of the next code, not consumed.  A reader that takes bit after bit runs out of
        bits exactly where no code begins fewer than 16 remaining bits, or the code is longer than what remains"""
        left = self.nbits - self.pos
        e = lut[self.peek16()]
        if e == 0:
            return (BAD_CODE if left >= 16 else TRUNCATED), 0, 0
        return (TRUNCATED if (e >> 8) > left else 0), e >> 8, e & 255

    def receive(self, size):
        if size == 0:
            return 0
        v = self.peek16() >> (16 - size)
        self.pos += size
        return v if v >> (size - 1) else v - (1 << size) + 1


def decode_block(bits, dc, ac, pred):
    """(status, the 64 coefficients in natural order or None, the DC predictor) of the next block.  The checks come
    in this order: the Huffman step, the symbol, the index, the magnitude bits, the DC range."""
    st, length, sym = bits.symbol(dc)
    if st:
        return st, None, pred
    if sym > 11:
        return BAD_CODE, None, pred
    if length + sym > bits.nbits - bits.pos:
        return TRUNCATED, None, pred
    bits.pos += length
    pred += bits.receive(sym)
    if not -2048 <= pred <= 2047:
        return BAD_CODE, None, pred
    block = [0] * 64
    block[0] = pred
    k = 1
    while k < 64:
        st, length, sym = bits.symbol(ac)
        if st:
            return st, None, pred
        run, size = sym >> 4, sym & 15
        if size == 0:
            if run == 0:
                bits.pos += length
                break
            if run != 15:
                return BAD_CODE, None, pred
            k += 16
            if k > 64:
                return OVERRUN, None, pred
            bits.pos += length
            continue
        if size > 10:
            return BAD_CODE, None, pred
        k += run
        if k > 63:
            return OVERRUN, None, pred
        if length + size > bits.nbits - bits.pos:
            return TRUNCATED, None, pred
        bits.pos += length
        block[int(J.ZIGZAG[k])] = bits.receive(size)
        k += 1
    return 0, block, pred


_ZZ = [int(v) for v in J.ZIGZAG]


def mcu_blocks(hv, c=3):
    """the blocks of an MCU in coding order: [(component, block row in the MCU, block column in the MCU)]; the MCU of
    a 1-component frame is its one block"""
    if c == 1:
        return [(0, 0, 0)]
    return [(0, v, u) for v in range(hv[1]) for u in range(hv[0])] + [(1, 0, 0), (2, 0, 0)]


def decode_coefficients(data, head=None, ret_segments=False):
    """(the int64 quantised coefficients in natural order, the status word).  The coefficients of a 1 x 1 or
    1-component frame are one (c, by, bx, 64) array; those of luma H x V are [Y (my * V, mx * H, 64), Cb (my, mx, 64),
    Cr (my, mx, 64)].  After an error the block where it happened and every later block of the segment are zero,
    earlier blocks of the same MCU keep their coefficients; the blocks of a missing segment are zero.
    ret_segments: also per segment None (missing) or (status bit or 0, the MCU of the error or None, the index of
    the block in that MCU or None)"""
    data = bytes(data)
    head = head or parse_header(data)
    c, ri, (hh, vv) = head["c"], head["ri"], head["sampling"]
    my, mx = -(-head["h"] // (8 * vv)), -(-head["w"] // (8 * hh))
    segs, status = split_segments(data, head["scan_begin"], head["nseg"])
    luts = [(_lut(dc), _lut(ac)) for dc, ac in head["huff"]]
    coefs = [np.zeros((my * vv, mx * hh, 64), np.int64)] + [np.zeros((my, mx, 64), np.int64) for _ in range(c - 1)]
    walk, report = mcu_blocks((hh, vv), c), []
    for j, seg in enumerate(segs):
        report.append(None if seg is None else (0, None, None))
        if seg is None:
            continue
        bits, pred = _Bits(unstuffed(data, *seg)), [0] * c
        dead = False
        for m in range(j * ri, min((j + 1) * ri, my * mx)):
            row, col = m // mx, m % mx
            for k, (comp, v, u) in enumerate(walk):
                st, block, pred[comp] = decode_block(bits, luts[comp][0], luts[comp][1], pred[comp])
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
    coefs = np.stack(coefs) if (hh, vv) == (1, 1) else coefs
    return (coefs, status, report) if ret_segments else (coefs, status)


# ------------------------------------------------------------------------------------------------ reconstruction
def dequantised(coefs, qtables):
    """(clamp(coef * Q, -2048, 2047) as (c, by, bx, 8, 8) [v][k], whether the clamp was active)"""
    raw = coefs * np.asarray(qtables, np.int64)[:, None, None, :]
    f = np.clip(raw, -2048, 2047)
    return f.reshape(f.shape[:3] + (8, 8)), bool((f != raw).any())


def integer_planes(f):
    """the pinned inverse transform: (c, by * 8, bx * 8) samples 0 .. 255"""
    t, _ = J.dct_matrix()
    g = (np.einsum("vy,cabvk->cabyk", t, f) + (1 << (SHIFT1 - 1))) >> SHIFT1
    s = (np.einsum("kn,cabyk->cabyn", t, g) + (1 << (SHIFT2 - 1))) >> SHIFT2
    c, by, bx = f.shape[:3]
    return np.clip(s + 128, 0, 255).transpose(0, 1, 3, 2, 4).reshape(c, by * 8, bx * 8)


def float_planes(f):
    """the float64 IDCT of the same dequantised coefficients, rounded and clipped"""
    _, a = J.dct_matrix()
    x = np.einsum("vy,cabvk,kn->cabyn", a, f.astype(np.float64), a) + 128
    c, by, bx = f.shape[:3]
    return np.clip(np.rint(x), 0, 255).astype(np.int64).transpose(0, 1, 3, 2, 4).reshape(c, by * 8, bx * 8)


def rgb_of(planes):
    y, cb, cr = planes[0], planes[1] - 128, planes[2] - 128
    return np.stack([np.clip(y + ((91881 * cr + 32768) >> 16), 0, 255),
                     np.clip(y - ((22554 * cb + 46802 * cr + 32768) >> 16), 0, 255),
                     np.clip(y + ((116130 * cb + 32768) >> 16), 0, 255)], axis=-1)


def ideal_rgb_of(planes):
    y, cb, cr = (p.astype(np.float64) for p in (planes[0], planes[1] - 128, planes[2] - 128))
    rgb = np.stack([y + 1.402 * cr, y - 0.344136 * cb - 0.714136 * cr, y + 1.772 * cb], axis=-1)
    return np.clip(np.rint(rgb), 0, 255)


def decode(data, head=None):
    """(the frame, uint8 (h, w) or (h, w, 3) RGB; the status word) of one stored file"""
    head = head or parse_header(data)
    coefs, status = decode_coefficients(data, head)
    planes = integer_planes(dequantised(coefs, head["qtables"])[0])[:, :head["h"], :head["w"]]
    frame = planes[0] if head["c"] == 1 else rgb_of(planes)
    return frame.astype(np.uint8), status


def ideal_decode(data, head=None):
    """dequantise, float64 IDCT, round and clip, JFIF inverse matrix in float64, round and clip: what
    jpeg_checks.ideal_decode computes, for any stream the decoder takes"""
    head = head or parse_header(data)
    coefs, _ = decode_coefficients(data, head)
    planes = float_planes(dequantised(coefs, head["qtables"])[0])[:, :head["h"], :head["w"]]
    return (planes[0] if head["c"] == 1 else ideal_rgb_of(planes)).astype(np.uint8)


def header_key(head):
    """what two frames must share to go into one call"""
    return (head["h"], head["w"], head["c"], head["ri"], head["qtables"].tobytes(),
            tuple((tuple(dc[0]), tuple(dc[1]), tuple(ac[0]), tuple(ac[1])) for dc, ac in head["huff"]),
            tuple(head["sampling"]))


# ------------------------------------------------------------------------------------------------ the host shim
def build_shim(root, out_dir):
    """tests/jpeg_decode_shim.cpp compiled for the host with -fsanitize=address,undefined into a stand-alone program:
    its path"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "llvm", "bin", "clang++")
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or (
        rocm_clang if os.path.exists(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler: neither g++, c++ or clang++ on the PATH nor %s" % rocm_clang
    exe = os.path.join(str(out_dir), "jpeg_decode_shim")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(root, "video-analysis_amd", "csrc"),
                           os.path.join(root, "tests", "jpeg_decode_shim.cpp"), "-o", exe])
    return exe


def shim_record(data, head, table):
    """one record of the shim's input: `data` under the header `head`; table(BITS, HUFFVAL) is a HuffDecode's bytes"""
    tables = b"".join(table(*dc) + table(*ac) for dc, ac in head["huff"])
    return (struct.pack("<8i", head["h"], head["w"], head["c"], head["ri"], head["scan_begin"], len(data),
                        *head["sampling"]) + head["qtables"].tobytes() + tables + data)


def run_shim(exe, records):
    """the lines the program prints for the records, one each"""
    run = subprocess.run([exe], input=b"".join(records), capture_output=True)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    return run.stdout.decode().split("\n")[:-1]


def shim_line(pixels, status):
    """the line of a record that decodes to these pixels and this status word: the status and the 64-bit FNV-1a hash"""
    h = 1469598103934665603
    for v in pixels.tobytes():
        h = ((h ^ v) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%d %d" % (status, h)
