"""The optimised Huffman tables of DESIGN.md §9, "Optimised Huffman tables", restated in Python: this file is the
definition, and the device equals it byte for byte.

  counts    freq[class][dc | ac][256], class 0 luma, 1 Cb and Cr: one count wherever the plain encoder looks up a code,
            over every block of every frame of the call
  a table   libjpeg's jpeg_gen_optimal_table (T.81 K.2 with symbol 256 reserved), written out literally with its
            `others` chains, without its limits on a count (10^9) and on a size before the limit to 16 (32)
  a stream  the plain stream (jpeg_checks, jpeg_sampled_encode_checks) with the computed (BITS, HUFFVAL) in its DHT
            segments and their codes in its entropy segments; nothing else changes

Everything that does not change is jpeg_checks' and jpeg_sampled_encode_checks': the plain encoders run here with
their segment coder replaced, once to collect the blocks and once to code them with the new tables.  Also the reader
of the fixture tests/golden/mjpeg_optimized_v1.npz.  Nothing here imports the package."""
import contextlib
import heapq

import numpy as np

import jpeg_checks as J
import jpeg_decode_checks as D
import jpeg_sampled_encode_checks as E

KEYS = (0x00, 0x10, 0x01, 0x11)         # the DHT byte of table t = 2 * class + ac: the order of the header and the ABI
TABLE_BYTES = 16 + 256                  # one table at the ABI: BITS, then HUFFVAL with the unused entries 0
LAYOUTS = (("mono", None), ("444", (1, 1)), ("422", (2, 1)), ("420", (2, 2)))
SHAPES = ((1, 1), (8, 8), (7, 9), (16, 16), (17, 33), (37, 53))
WIDE = {"mono": (8, 264), "444": (8, 264), "422": (8, 392), "420": (16, 272)}    # more than one chunk per segment
QUALITIES = (1, 50, 90, 100)


# ------------------------------------------------------------------------------------------------ one table
def gen_optimal_table(freq):
    """(BITS, 16 entries; HUFFVAL) of 256 counts.  Counts that are all 0 give an empty table."""
    freq = [int(v) for v in freq] + [1]
    assert len(freq) == 257 and min(freq) >= 0
    codesize, others = [0] * 257, [-1] * 257
    while True:
        c1, v = -1, None
        for i in range(257):
            if freq[i] and (v is None or freq[i] <= v):
                c1, v = i, freq[i]
        c2, v = -1, None
        for i in range(257):
            if freq[i] and i != c1 and (v is None or freq[i] <= v):
                c2, v = i, freq[i]
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    top = max(codesize)
    bits = [0] * (max(top, 16) + 1)
    for s in codesize:
        if s:
            bits[s] += 1
    for i in range(top, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while i > 0 and bits[i] == 0:
        i -= 1
    if i > 0:
        bits[i] -= 1
    vals = [j for s in range(1, top + 1) for j in range(256) if codesize[j] == s]
    assert sum(bits[1:17]) == len(vals)
    return bits[1:17], vals


def table_bytes(bits, vals):
    """one table as the ABI returns it: TABLE_BYTES uint8"""
    return np.array(list(bits) + list(vals) + [0] * (256 - len(vals)), np.uint8)


def table_from_lengths(lengths):
    """the table whose 256 symbols have these code lengths (0: no code): HUFFVAL lists them by length, then value"""
    lengths = [int(v) for v in lengths]
    return table_bytes([lengths.count(s) for s in range(1, 17)],
                       [j for s in range(1, 17) for j in range(256) if lengths[j] == s])


def unpacked_tables(z, part):
    """the tables (t, TABLE_BYTES) of a part of the fixture: stored as the code length of every symbol, and in full
    where the lengths do not give the table back"""
    out = np.stack([table_from_lengths(row) for row in z[part + "_tables_lengths"]])
    for k, full in zip(z[part + "_tables_odd"], z[part + "_tables_full"]):
        out[int(k)] = full
    return out


def code_lengths(bits, vals):
    """{symbol: length}"""
    return {sym: length for sym, (_, length) in J.huffman_codes(list(bits), list(vals)).items()}


def heap_cost(freq):
    """(the cost sum(freq * size) of a Huffman tree over the 257 symbols, the reserved one with its count of 1
    included; the depth of that tree): an independent construction"""
    freq = [int(v) for v in freq]
    heap = [(f, i, (i,)) for i, f in enumerate(freq + [1]) if f]
    heapq.heapify(heap)
    depth = dict.fromkeys(range(257), 0)
    tick = 257
    while len(heap) > 1:
        fa, _, a = heapq.heappop(heap)
        fb, _, b = heapq.heappop(heap)
        for i in a + b:
            depth[i] += 1
        heapq.heappush(heap, (fa + fb, tick, a + b))
        tick += 1
    return sum(f * depth[i] for i, f in enumerate(freq + [1])), max(depth.values())


# ------------------------------------------------------------------------------------------------ counts
def block_counts(blocks, comp_of_block, freq):
    """adds the symbols of one entropy segment to freq (2, 2, 256) int64.  blocks: (B, 64) zigzag coefficients in
    coding order; the DC predictors start at 0"""
    pred = {}
    for block, comp in zip(np.asarray(blocks, np.int64), comp_of_block):
        t = min(int(comp), 1)
        diff = int(block[0]) - pred.get(int(comp), 0)
        pred[int(comp)] = int(block[0])
        freq[t, 0, abs(diff).bit_length()] += 1
        run = 0
        for v in block[1:]:
            v = int(v)
            if v == 0:
                run += 1
                continue
            freq[t, 1, 0xF0] += run >> 4
            freq[t, 1, ((run & 15) << 4) | abs(v).bit_length()] += 1
            run = 0
        if block[63] == 0:
            freq[t, 1, 0] += 1


def file_counts(data, head=None):
    """the counts (2, 2, 256) recovered from one stored baseline file of any restart interval, and its four tables
    {key: (BITS, HUFFVAL)}"""
    head = head or D.parse_header(data, "any")
    coefs, status = D.decode_coefficients(data, head)
    assert status == 0
    c, ri, (hh, vv) = head["c"], head["ri"], head["sampling"]
    my, mx = -(-head["h"] // (8 * vv)), -(-head["w"] // (8 * hh))
    walk = D.mcu_blocks((hh, vv), c)
    freq = np.zeros((2, 2, 256), np.int64)
    for m0 in range(0, my * mx, ri):
        blocks, comps = [], []
        for m in range(m0, min(m0 + ri, my * mx)):
            row, col = divmod(m, mx)
            for comp, v, u in walk:
                nat = coefs[0][row * vv + v, col * hh + u] if comp == 0 else coefs[comp][row, col]
                blocks.append(nat[J.ZIGZAG])
                comps.append(comp)
        block_counts(blocks, comps, freq)
    tables = {}
    for k, (dc, ac) in enumerate(head["huff"]):
        tables[min(k, 1)], tables[0x10 | min(k, 1)] = dc, ac
    return freq, tables


# ------------------------------------------------------------------------------------------------ a stream
@contextlib.contextmanager
def _replaced(name, value):
    old = getattr(J, name)
    setattr(J, name, value)
    try:
        yield
    finally:
        setattr(J, name, old)


def _plain(frames, quality, sampling):
    frames = np.asarray(frames)
    if frames.ndim == 3 or tuple(sampling or (1, 1)) == (1, 1):
        return J.encode(frames, quality)
    return E.encode(frames, quality, sampling)


def call_counts(frames, quality=90, sampling=None):
    """the counts (2, 2, 256) of one call: frames (n, h, w) or (n, h, w, 3), sampling None or (1, 1), (2, 1), (2, 2)"""
    freq = np.zeros((2, 2, 256), np.int64)

    def collect(blocks, comp_of_block):
        block_counts(blocks, comp_of_block, freq)
        return np.zeros(0, np.uint8)
    with _replaced("encode_segment", collect):
        _plain(frames, quality, sampling)
    return freq


def tables_of(freq, c):
    """[(BITS, HUFFVAL)] of the counts of a call, in the order KEYS: two tables for c = 1, four for c = 3"""
    return [gen_optimal_table(freq[t >> 1, t & 1]) for t in range(2 if c == 1 else 4)]


def split_header(head):
    """(the bytes in front of the DHT segments, the bytes behind them) of a plain header"""
    segs, at = [], 2
    while at < len(head):
        size = (head[at + 2] << 8) | head[at + 3]
        segs.append((head[at + 1], at, at + 2 + size))
        at += 2 + size
    dht = [s for s in segs if s[0] == 0xC4]
    assert dht and [s[0] for s in segs[segs.index(dht[0]):segs.index(dht[-1]) + 1]] == [0xC4] * len(dht)
    return bytes(head[:dht[0][1]]), bytes(head[dht[-1][2]:])


def header_with(plain_head, tables):
    pre, post = split_header(plain_head)
    return pre + b"".join(J._segment(0xC4, bytes([key] + list(bits) + list(vals)))
                          for key, (bits, vals) in zip(KEYS, tables)) + post


def encode(frames, quality=90, sampling=None):
    """(the files of one call as a list of bytes, its tables as (t, TABLE_BYTES) uint8)"""
    frames = np.asarray(frames)
    c = 1 if frames.ndim == 3 else 3
    if len(frames) == 0:
        return [], np.zeros((2 if c == 1 else 4, TABLE_BYTES), np.uint8)
    tables = tables_of(call_counts(frames, quality, sampling), c)
    codes = dict(J._CODES)
    for key, (bits, vals) in zip(KEYS, tables):
        code, length = np.zeros(256, np.int64), np.zeros(256, np.int64)
        for sym, (cd, n) in J.huffman_codes(bits, vals).items():
            code[sym], length[sym] = cd, n
        codes[key] = (code, length)
    with _replaced("_CODES", codes):
        files = _plain(frames, quality, sampling)
    plain_head = J.header(*frames.shape[1:3], c, quality)
    nhead = len(plain_head)
    out = []
    for f in files:
        out.append(header_with(f[:nhead], tables) + f[nhead:])
    return out, np.stack([table_bytes(*t) for t in tables])


# ------------------------------------------------------------------------------------------------ pictures
def frame_of(content, h, w, c, rng):
    """the fixture's and the GPU tests' pictures; `rng` is drawn from for noise only"""
    if c == 3:
        return E.frame_of(content, h, w, rng)
    if content == "noise":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    if content == "ramp":
        yy, xx = np.mgrid[:h, :w]
        return ((xx + yy) * 255 // max(h + w - 2, 1)).astype(np.uint8)
    return np.full((h, w), 0 if content == "zeros" else 255, np.uint8)


def stack_of(n, h, w, c, seed):
    """n = 1: noise; n = 3: a constant-0 frame, a noise frame and a ramp"""
    rng = np.random.default_rng(seed)
    contents = ("noise",) if n == 1 else ("zeros", "noise", "ramp")
    return np.stack([frame_of(k, h, w, c, rng) for k in contents])


def long_run_stack():
    """4 monochrome frames of 256 x 256 for quality 90: three of uniform noise, whose 3072 blocks make every other symbol
    frequent, and a grey frame whose first block is the highest basis function, one coefficient behind a run of 62.
    ZRL is counted 3 times in the call and gets a code of 16 bits, so that coefficient adds 3 * 16 + its code + its
    magnitude bits: more than 64 (long_run_bits says how many)"""
    rng = np.random.default_rng(7477)
    stack = rng.integers(0, 256, (4, 256, 256), dtype=np.uint8)
    stack[3] = 128
    c = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    stack[3, :8, :8] = np.rint(128 + 127 * np.outer(c, c))
    return stack


def long_run_bits(stack, quality, tables):
    """(the length of the ZRL code, the most bits one coefficient of a monochrome call adds) under its tables"""
    dc, ac = (code_lengths(t[:16], t[16:16 + int(t[:16].sum())]) for t in tables[:2])
    most = 0
    for frame in stack:
        for block in J.frame_coefficients(frame, quality)[0].reshape(-1, 64):
            at = 0
            for k in np.flatnonzero(block[1:]) + 1:
                run, size = int(k) - at - 1, abs(int(block[k])).bit_length()
                most = max(most, (run >> 4) * ac[0xF0] + ac[((run & 15) << 4) | size] + size)
                at = int(k)
    return ac.get(0xF0, 0), most


def chosen_counts():
    """[(name, 256 counts)]: fixture part 2"""
    out = [("one_symbol", {5: 7}), ("two_symbols", {3: 9, 200: 2}), ("equal_256", {i: 1000 for i in range(256)}),
           ("ones_256", {i: 1 for i in range(256)}),
           ("dc_shape", dict(zip(range(12), (5000, 9000, 7000, 4000, 2500, 1200, 600, 300, 120, 40, 9, 2))))]
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    out.append(("fibonacci_40", {3 * i + 1: f for i, f in enumerate(fib)}))
    out.append(("powers_40", {5 * i + 2: 1 << i for i in range(40)}))
    rng = np.random.default_rng(2026)
    named = []
    for name, sparse in out:
        freq = np.zeros(256, np.int64)
        for i, f in sparse.items():
            freq[i] = f
        named.append((name, freq))
    for k in range(200):
        freq = rng.integers(0, 1 << int(rng.integers(1, 40)), 256, dtype=np.int64)
        freq[rng.random(256) < rng.random()] = 0
        named.append(("random_%03d" % k, freq))
    return named


# ------------------------------------------------------------------------------------------------ the fixture
def fixture(path):
    """tests/golden/mjpeg_optimized_v1.npz as a dict:
      pin     [(name, counts (4, 256) int64, tables (4, TABLE_BYTES) as the file's own DHT gives them)], monochrome: 2
      chosen  [(name, counts (256,) as chosen_counts() draws them, the restatement's table (TABLE_BYTES,))]
      calls   [(name, layout name, quality, frames, [the optimised files], tables, Pillow's decode of every file as its
              int8 difference from jpeg_subsampled_checks.ideal_decode of the file: pillow_pixels(call) adds it again)]
      ratios  {name: (Pillow's plain bytes, Pillow's optimised bytes)} of the benchmark's pictures"""
    z = np.load(path, allow_pickle=False)
    out = {"pin": [], "chosen": [], "calls": [], "ratios": {}}
    pin, chosen_tables, call_tables = (unpacked_tables(z, part) for part in ("pin", "chosen", "call"))
    at = 0
    for name, t in zip(z["pin_names"], z["pin_tables_of"]):
        t = int(t)
        out["pin"].append((str(name), z["pin_counts"][at:at + t].astype(np.int64), pin[at:at + t]))
        at += t
    chosen = chosen_counts()
    assert [name for name, _ in chosen] == [str(name) for name in z["chosen_names"]]
    for (name, freq), table in zip(chosen, chosen_tables):
        out["chosen"].append((name, freq, table))
    stacks, at = {}, 0
    for n, h, w, c in z["stack_shapes"]:
        shape = (int(n), int(h), int(w)) + ((3,) if c == 3 else ())
        size = int(np.prod(shape))
        stacks[(int(n), int(h), int(w), int(c))] = z["stack_frames"][at:at + size].reshape(shape)
        at += size
    bat = pat = tat = k0 = 0
    for name, layout, quality, key in zip(z["call_names"], z["call_layouts"], z["call_quality"], z["call_shapes"]):
        frames = stacks[tuple(int(v) for v in key)]
        n, t = len(frames), 2 if frames.ndim == 3 else 4
        files, seen = [], []
        for k in range(k0, k0 + n):
            files.append(z["call_blob"][bat:bat + int(z["call_sizes"][k])].tobytes())
            bat += int(z["call_sizes"][k])
            diff = z["call_pillow_diff"][pat:pat + frames[0].size].reshape(frames[0].shape)
            pat += frames[0].size
            seen.append(diff)
        k0 += n
        out["calls"].append((str(name), str(layout), int(quality), frames, files, call_tables[tat:tat + t],
                             np.stack(seen)))
        tat += t
    for name, sizes in zip(z["ratio_names"], z["ratio_bytes"]):
        out["ratios"][str(name)] = (int(sizes[0]), int(sizes[1]))
    return out, z


def pillow_pixels(call):
    """what Pillow decoded from a call's files when the fixture was written"""
    import jpeg_subsampled_checks as S
    return np.stack([(S.ideal_decode(f).astype(np.int16) + d).astype(np.uint8) for f, d in zip(call[4], call[6])])
