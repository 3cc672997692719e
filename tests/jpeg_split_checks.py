"""The scan of DESIGN.md §9, "Split Motion-JPEG decoding", restated in Python on the raw bytes of a frame's one entropy
segment: this file is the definition of the states, of the scan step with its recovery rule, of the rounds and of the
entry states they converge to.  The device and the host shim (tests/jpeg_split_shim.cpp) equal it exactly; the pixels
and status words stay those of jpeg_decode_checks / jpeg_subsampled_checks.  Nothing here imports the package."""
import os
import shutil
import struct
import subprocess

import numpy as np

import jpeg_checks as J
import jpeg_decode_checks as D

END = None                      # the state behind a symbol that needs bits beyond the segment's end


class Segment(object):
    """the one segment [b, e) of a file without restart markers, its tables and its MCU walk"""

    def __init__(self, data, head=None):
        self.data = bytes(data)
        self.head = head or D.parse_header(self.data, sampling="any")
        segs, self.marker = D.split_segments(self.data, self.head["scan_begin"], 1)
        self.b, self.e = segs[0]
        raw = np.frombuffer(self.data, np.uint8)[self.b:self.e]
        # a byte is stuffing iff it is 00, not the segment's first, and the byte before it is FF
        stuffing = np.zeros(len(raw), bool)
        if len(raw) > 1:
            stuffing[1:] = (raw[1:] == 0) & (raw[:-1] == 0xFF)
        self.stuffing = stuffing
        self.raw_of = [int(v) + self.b for v in np.flatnonzero(~stuffing)] + [self.e]   # unstuffed index -> raw offset
        self.index_of = (np.cumsum(~stuffing) - 1).tolist()                             # raw offset - b -> unstuffed
        self.bits = D._Bits(raw[~stuffing].tobytes())
        self.luts = [(D._lut(dc), D._lut(ac)) for dc, ac in self.head["huff"]]
        self.walk = D.mcu_blocks(tuple(self.head["sampling"]), self.head["c"])
        hh, vv = self.head["sampling"]
        self.my, self.mx = -(-self.head["h"] // (8 * vv)), -(-self.head["w"] // (8 * hh))
        self.total = self.my * self.mx * len(self.walk)
        self.steps = {}

    def lanes(self, sub):
        n = self.e - self.b
        return -(-n // sub) if n > sub else 1

    def stop(self, i, sub):
        return self.e if i + 1 == self.lanes(sub) else self.b + (i + 1) * sub

    def guess(self, i, sub):
        at = self.b + i * sub
        return (at + 1 if self.stuffing[at - self.b] else at, 0, 0, 0)

    def step(self, state):
        """the scan step: (the next state or END, (natural index, value) or None, whether the step failed)"""
        if state not in self.steps:                     # the rounds walk the same states again and again
            self.steps[state] = self._step(state)
        return self.steps[state]

    def _step(self, state):
        q, bit, k, z = state
        bits = self.bits
        bits.pos = 8 * self.index_of[q - self.b] + bit if q < self.e else bits.nbits
        left = bits.nbits - bits.pos
        dc, ac = self.luts[self.walk[k][0]]
        st, length, sym = bits.symbol(ac if z else dc)
        if st == D.TRUNCATED:
            return END, None, True
        failed, value = bool(st), None
        if st:
            pass
        elif z == 0:
            if sym > 11:
                failed = True
            elif length + sym > left:
                return END, None, True
            else:
                bits.pos += length
                value, z = (0, bits.receive(sym)), 1
        else:
            run, size = sym >> 4, sym & 15
            if size == 0:
                if run == 0:
                    bits.pos += length
                    z = 64
                elif run != 15 or z + 16 > 64:
                    failed = True
                else:
                    bits.pos += length
                    z += 16
            elif size > 10 or z + run > 63:
                failed = True
            elif length + size > left:
                return END, None, True
            else:
                bits.pos += length
                value, z = (int(J.ZIGZAG[z + run]), bits.receive(size)), z + run + 1
        if failed:
            bits.pos += 1
            z = 0
        if z == 64:
            k, z = (k + 1) % len(self.walk), 0
        return (self.raw_of[bits.pos >> 3], bits.pos & 7, k, z), value, failed

    def run(self, entry, stop):
        """the exit of a lane that enters with `entry` and steps while its state lies in front of `stop`"""
        state = entry
        while state is not END and state[0] < stop:
            state = self.step(state)[0]
        return state


def serial_walk(seg):
    """the serial decoder on the same step: (every state it stands in, in order; the coefficients (blocks, 64) of the
    blocks it completes before its first failure or the frame's end)"""
    state, states = (seg.b, 0, 0, 0), []
    coefs, block, dead, pred = [], [0] * 64, False, [0] * seg.head["c"]
    while state is not END and state[0] < seg.e:
        states.append(state)
        nxt, value, failed = seg.step(state)
        dead = dead or failed or len(coefs) == seg.total
        if not dead:
            if value is not None and value[0] == 0 and state[3] == 0:
                comp = seg.walk[state[2]][0]
                pred[comp] += value[1]
                value = (0, pred[comp])
            if value is not None:
                block[value[0]] = value[1]
            if nxt is not END and nxt[3] == 0:
                coefs.append(block)
                block = [0] * 64
        state = nxt
    states.append(state)
    return states, np.array(coefs, np.int64).reshape(-1, 64)


def scan(seg, sub):
    """the rounds of the scan with subsequences of `sub` raw bytes: (rounds, the entry states it converges to).  Round
    1 runs every lane, lane 0 from the truth and the others from their guesses; round r + 1 gives lane i the exit of
    lane i - 1 of round r and runs the lanes whose entry changed; `rounds` is the last round in which a lane ran."""
    lanes = seg.lanes(sub)
    entries = [(seg.b, 0, 0, 0)] + [seg.guess(i, sub) for i in range(1, lanes)]
    exits, changed, rounds = [END] * lanes, list(range(lanes)), 0
    while changed:
        rounds += 1
        for i in changed:
            exits[i] = seg.run(entries[i], seg.stop(i, sub))
        changed = [i for i in range(1, lanes) if exits[i - 1] != entries[i]]
        for i in changed:                               # all from the exits of this round: Jacobi
            entries[i] = exits[i - 1]
    return rounds, entries


def chain_entries(seg, sub, states):
    """what the entries must be: the first state of the serial chain in or behind each subsequence"""
    out, at = [], 0
    for i in range(seg.lanes(sub)):
        first = seg.b + i * sub
        while states[at] is not END and states[at][0] < first:
            at += 1
        out.append(states[at])
    return out


def serial_coefficients(seg, coefs=None):
    """the coefficients of jpeg_decode_checks.decode_coefficients (`coefs` where the caller has them) in decode order,
    (blocks, 64)"""
    if coefs is None:
        coefs, _ = D.decode_coefficients(seg.data, seg.head)
    hh, vv = seg.head["sampling"]
    out = []
    for m in range(seg.my * seg.mx):
        row, col = divmod(m, seg.mx)
        for comp, v, u in seg.walk:
            out.append(coefs[comp][row * vv + v, col * hh + u] if comp == 0 else coefs[comp][row, col])
    return np.array(out, np.int64).reshape(-1, 64)


# ------------------------------------------------------------------------------------------------ streams for tests
LAYOUTS = ("mono", "444", "422", "420")
_SAMPLING = {"422": (2, 1), "420": (2, 2)}


def encode_plain(frame, layout, quality=100):
    """one baseline JFIF file without DRI and without restart markers from the restated encoders: `frame` is (h, w, 3)
    uint8, of which "mono" takes the green plane"""
    import jpeg_subsampled_checks as S
    frame = np.asarray(frame)
    if layout in _SAMPLING:
        return S.encode_frame(frame, quality, _SAMPLING[layout], ri=0)
    frame = frame[..., 1] if layout == "mono" else frame
    h, w = frame.shape[:2]
    coefs = J.frame_coefficients(frame, quality)
    c = len(coefs)
    head = _without_dri(J.header(h, w, c, quality))
    blocks = np.stack([co.reshape(-1, 64) for co in coefs], axis=1).reshape(-1, 64)        # MCU by MCU
    body = J.encode_segment(blocks, np.tile(np.arange(c), len(blocks) // c)).tobytes()
    return head + body + b"\xff\xd9"


def _without_dri(head):
    at = len(head) - (20 if head[-20:-18] == b"\xff\xdd" else 16)
    assert head[at:at + 4] == b"\xff\xdd\x00\x04" and head[at + 6:at + 8] == b"\xff\xda"
    return head[:at] + head[at + 6:]


def picture(h, w, seed, sigma=6.0):
    """a smooth ramp with discs and Gaussian noise, (h, w, 3) uint8"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    base = np.stack([40 + 150 * xx / w, 200 - 120 * yy / h, 90 + 60 * (xx + yy) / (h + w)], axis=-1)
    for _ in range(4):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(3, max(4, min(h, w) / 4))
        base[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] += rng.uniform(-80, 80, 3)
    return np.clip(base + rng.normal(0, sigma, base.shape), 0, 255).astype(np.uint8)


def restartless(streams):
    """[(name, data, head)] of those of [(name, data)] that have one segment"""
    out = []
    for name, data in streams:
        head = D.parse_header(data, sampling="any")
        if head["nseg"] == 1:
            out.append((name, data, head))
    return out


def fixture_streams(root):
    """the valid streams of one segment of tests/golden/mjpeg_decode_v1.npz (with mjpeg_v1.npz) and
    mjpeg_subsampled_v1.npz: [(name, data, head)]"""
    import jpeg_subsampled_checks as S
    golden = os.path.join(root, "tests", "golden")
    enc = np.load(os.path.join(golden, "mjpeg_v1.npz"), allow_pickle=False)
    dec = np.load(os.path.join(golden, "mjpeg_decode_v1.npz"), allow_pickle=False)
    cases, _ = S.fixture_cases(os.path.join(golden, "mjpeg_subsampled_v1.npz"))
    streams = [("a " + str(n), enc["bytes_" + str(n)].tobytes()) for n in dec["names_a"]]
    streams += [("b " + str(n), dec["b_bytes_" + str(n)].tobytes()) for n in dec["names_b"]]
    streams += [(name, data) for name, data, _, _ in cases["a"]]
    return restartless(streams)


def layout_of(head):
    return "mono" if head["c"] == 1 else {(1, 1): "444", (2, 1): "422", (2, 2): "420"}[tuple(head["sampling"])]


def hostile_streams(data, seed):
    """[(name, bytes)] made from the valid stream `data` of one segment, all under its header: a cut at every byte of
    the last 40, cuts exactly behind a complete block with blocks missing, 64 single-bit flips, a run of FF 00"""
    seg = Segment(data)
    out = [("cut -%d" % j, data[:len(data) - j]) for j in range(1, 41)]
    states, _ = serial_walk(seg)
    ends = [s[0] for s in states[1:] if s is not END and s[1] == 0 and s[3] == 0 and seg.b < s[0] < seg.e - 8]
    assert ends, "no block of this stream ends on a byte boundary"
    out += [("cut behind a block at %d" % q, data[:q]) for q in (ends[0], ends[len(ends) // 2], ends[-1])]
    rng = np.random.default_rng(seed)
    for at in rng.integers(8 * seg.b, 8 * seg.e, 64):
        flipped = bytearray(data)
        flipped[at >> 3] ^= 0x80 >> (at & 7)
        out.append(("flip %d" % at, bytes(flipped)))
    out.append(("ff00", data[:seg.b] + b"\xff\x00" * ((seg.e - seg.b) // 2) + b"\xff\xd9"))
    return out


def dc_overrun_stream(seed=7, first=30):
    """a monochrome 64 x 48 stream whose DC values climb by 1000 a block from block `first` on: the DC value leaves
    -2048 .. 2047 a few blocks later, far behind the first subsequences; every symbol is a valid one"""
    frame = picture(48, 64, seed, 20.0)[..., 1]
    blocks = J.frame_coefficients(frame, 100)[0].reshape(-1, 64).copy()
    blocks[first:, 0] = blocks[first - 1, 0] + 1000 * np.arange(1, len(blocks) - first + 1)
    blocks[first + 4:, 0] = blocks[first + 3, 0]
    body = J.encode_segment(blocks, np.zeros(len(blocks), np.int64)).tobytes()
    return _without_dri(J.header(48, 64, 1, 100)) + body + b"\xff\xd9"


# ------------------------------------------------------------------------------------------------ the host shim
def build_shim(root, out_dir):
    """tests/jpeg_split_shim.cpp compiled for the host with -fsanitize=address,undefined into a stand-alone program:
    its path"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "llvm", "bin", "clang++")
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or (
        rocm_clang if os.path.exists(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler: neither g++, c++ or clang++ on the PATH nor %s" % rocm_clang
    exe = os.path.join(str(out_dir), "jpeg_split_shim")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(root, "video-analysis_amd", "csrc"),
                           os.path.join(root, "tests", "jpeg_split_shim.cpp"), "-o", exe])
    return exe


def shim_record(data, head, table, sub, max_rounds):
    """one record of the shim's input: jpeg_decode_checks.shim_record's with ri replaced by sub and max_rounds put in
    front"""
    tables = b"".join(table(*dc) + table(*ac) for dc, ac in head["huff"])
    return (struct.pack("<9i", head["h"], head["w"], head["c"], sub, head["scan_begin"], len(data),
                        head["sampling"][0], head["sampling"][1], max_rounds)
            + head["qtables"].tobytes() + tables + data)
