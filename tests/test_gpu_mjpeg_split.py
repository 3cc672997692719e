"""GPU: frames without restart markers through the split decoder (va_jpeg_decode_split_u8, ops.jpeg_decode(split=...)),
byte for byte against the serial restatement (tests/jpeg_decode_checks.py, tests/jpeg_subsampled_checks.py) and round
for round against the restated scan (tests/jpeg_split_checks.py); DESIGN.md §9, "Split Motion-JPEG decoding".  No
tolerances."""
import os

import numpy as np
import pytest

import jpeg_decode_checks as D
import jpeg_split_checks as P
import jpeg_subsampled_checks as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUBS = (16, 48, 256)
_MEMO = {}


def _decoded(data, head):
    """the serial restatement's (pixels, status) of a stream, computed once"""
    if data not in _MEMO:
        _MEMO[data] = S.decode(data, head)
    return _MEMO[data]


def _segment(data, head):
    if (data, "segment") not in _MEMO:
        _MEMO[data, "segment"] = P.Segment(data, head)
    return _MEMO[data, "segment"]


def _rounds(data, head, sub):
    """the restated scan's rounds of a stream, computed once"""
    if (data, sub) not in _MEMO:
        _MEMO[data, sub] = P.scan(_segment(data, head), sub)[0]
    return _MEMO[data, sub]


@pytest.fixture(scope="module")
def gpu():
    from video import _hip
    return _hip.lib()


@pytest.fixture(scope="module")
def valid():
    """{layout: [(name, data, head)]}: a spread of the fixtures' streams of one segment from 1 x 1 to 37 x 53, and
    64 x 48 frames of the restated encoders at quality 100.  One of the monochrome ones has entropy bytes that end
    exactly on a multiple of 48 (and so of 16)."""
    out = {layout: [] for layout in P.LAYOUTS}
    for item in P.fixture_streams(ROOT):
        out[P.layout_of(item[2])].append(item)
    for layout in P.LAYOUTS:
        items = sorted(out[layout], key=lambda it: (it[2]["h"] * it[2]["w"], it[0]))
        assert (items[0][2]["h"], items[0][2]["w"]) == (1, 1) and (items[-1][2]["h"], items[-1][2]["w"]) == (37, 53)
        out[layout] = items[:2] + items[2:-2:5] + items[-2:]
        for seed in (5, 6, 7):
            data = P.encode_plain(P.picture(48, 64, seed), layout)
            out[layout].append(("64x48 %s %d" % (layout, seed), data, D.parse_header(data, sampling="any")))
    for seed in range(1000):
        data = P.encode_plain(P.picture(48, 64, 100 + seed), "mono")
        head = D.parse_header(data, sampling="any")
        seg = P.Segment(data, head)
        if (seg.e - seg.b) % 48 == 0:
            out["mono"].append(("64x48 mono, %d entropy bytes" % (seg.e - seg.b), data, head))
            break
    else:
        raise AssertionError("no picture whose entropy bytes end on a multiple of 48")
    return out


@pytest.fixture(scope="module")
def hostile():
    """[(name, data, head of the stream it was made from)] per source stream, the DC run with the monochrome ones"""
    out = {}
    for layout, seed in (("420", 11), ("mono", 12)):
        data = P.encode_plain(P.picture(24, 40, seed, 12.0), layout, 90)
        head = D.parse_header(data, sampling="any")
        out[layout] = [("valid", data, head)] + [(name, bad, head) for name, bad in P.hostile_streams(data, seed)]
    data = P.dc_overrun_stream()
    out["dc"] = [("dc overrun", data, D.parse_header(data, sampling="any"))]
    return out


def _by_shape(items):
    groups = {}
    for item in items:
        groups.setdefault((item[2]["h"], item[2]["w"]), []).append(item)
    return list(groups.values())


def _check_batch(batch, sub, max_rounds, monkeypatch):
    """one ops.jpeg_decode call of frames of one shape: pixels and status the serial restatement's, rounds the restated
    scan's, -1 where it needs more than max_rounds"""
    from video import ops
    with monkeypatch.context() as patch:
        patch.setattr(ops, "JPEG_SPLIT_MAX_ROUNDS", max_rounds)
        got, status, rounds = ops.jpeg_decode([data for _, data, _ in batch], split=sub, ret_status=True,
                                              ret_rounds=True)
    assert got.dtype == np.uint8 and rounds.dtype == np.int32
    fell = 0
    for k, (name, data, head) in enumerate(batch):
        pixels, want_status = _decoded(data, head)
        assert status[k] == want_status, (name, sub, status[k], want_status)
        assert np.array_equal(got[k], pixels), (name, sub)
        want = _rounds(data, head, sub)
        assert rounds[k] == (want if want <= max_rounds else -1), (name, sub, max_rounds, rounds[k], want)
        fell += rounds[k] < 0
    return fell


@pytest.mark.parametrize("layout", P.LAYOUTS)
def test_valid_streams_equal_both_restatements(gpu, valid, layout, monkeypatch):
    """pixels, status and rounds at sub_bytes 16, 48 and 256 with as many rounds as the longest frame has
    subsequences, so that every frame converges"""
    lanes = 0
    for sub in SUBS:
        for batch in _by_shape(valid[layout]):
            most = max(_segment(data, head).lanes(sub) for _, data, head in batch)
            assert _check_batch(batch, sub, most, monkeypatch) == 0
            lanes = max(lanes, most)
    assert lanes >= 100
    if layout == "mono":
        name, data, head = valid[layout][-1]
        seg = _segment(data, head)
        assert (seg.e - seg.b) % 48 == 0 and seg.lanes(48) * 48 == seg.e - seg.b


@pytest.mark.parametrize("layout", P.LAYOUTS)
def test_forced_fallback_decodes_identically(gpu, valid, layout, monkeypatch):
    """max_rounds 0 (every frame falls back) and 1 (those of more than one round): -1 and the same bytes"""
    batch = _by_shape(valid[layout])[-1]                             # the 64 x 48 frames
    assert len(batch) >= 2
    one = [it for it in valid[layout] if _rounds(it[1], it[2], 256) == 1]
    assert one and any(_rounds(data, head, 16) > 1 for _, data, head in batch)
    assert _check_batch(batch, 16, 0, monkeypatch) == len(batch)
    assert _check_batch(batch, 16, 1, monkeypatch) >= 1
    for group in _by_shape(one):
        assert _check_batch(group, 256, 1, monkeypatch) == 0         # at max_rounds = 1 these do not fall back
        assert _check_batch(group, 256, 0, monkeypatch) == len(group)


def _abi_run(L, batch, sub, max_rounds, max_scan, workspace_bytes=None, fill=0xA5, extra=64):
    """va_jpeg_decode_split_u8 on raw buffers filled with `fill`: (pixels, status, rounds), each with `extra` bytes
    behind"""
    from video import _hip, ops
    heads = [ops.jpeg_parse_header(data, sampling="any") for data, _ in batch]
    head = heads[0]
    n, h, w, c = len(batch), head["h"], head["w"], head["c"]
    lh, lv = head["sampling"]
    tables = b"".join(ops._jpeg_decode_table(*dc) + ops._jpeg_decode_table(*ac) for dc, ac in head["huff"])
    offsets = np.concatenate([[0], np.cumsum([len(d) for d, _ in batch])]).astype(np.int64)
    ins = dict(bytes=np.frombuffer(b"".join(d for d, _ in batch), np.uint8), offsets=offsets,
               scan=np.array([hd["scan_begin"] for hd in heads], np.int64), qt=head["qtables"].ravel(),
               huff=np.frombuffer(tables, np.uint8))
    dev = {k: _hip.DeviceBuffer.from_array(v) for k, v in ins.items()}
    full = int(L.va_jpeg_decode_split_workspace_bytes(n, h, w, c, lh, lv, sub, max_scan))
    room = full if workspace_bytes is None else workspace_bytes
    outs = dict(out=n * h * w * c + extra, status=4 * n + extra, rounds=4 * n + extra, ws=room)
    for k, m in outs.items():
        dev[k] = _hip.DeviceBuffer(m)
        _hip.check(L.va_memset(dev[k].ptr, fill, dev[k].nbytes, None))
    try:
        _hip.check(L.va_jpeg_decode_split_u8(
            dev["bytes"].ptr, dev["offsets"].ptr, dev["scan"].ptr, n, h, w, c, lh, lv, dev["qt"].ptr, dev["huff"].ptr,
            len(tables), dev["out"].ptr, dev["status"].ptr, dev["ws"].ptr, room, sub, max_rounds, max_scan,
            dev["rounds"].ptr, None))
        return tuple(dev[k].download((outs[k],), np.uint8) for k in ("out", "status", "rounds"))
    finally:
        for b in dev.values():
            b.free()


def _check_abi(gpu, valid, hostile, fill):
    """through the raw ABI, on buffers and a workspace filled with a pattern: a batch that mixes frames that converge
    in max_rounds with ones that do not and with one longer than max_scan_bytes; the hostile streams between valid
    neighbours; chunks; two runs; the bytes behind every buffer"""
    frames = [(data, head) for name, data, head in valid["420"] if name.startswith("64x48")]
    lengths = [_segment(data, head).e - _segment(data, head).b for data, head in frames]
    longest = int(np.argmax(lengths))
    assert len(frames) == 3 and sorted(set(lengths)) == sorted(lengths)
    max_scan = max(n for k, n in enumerate(lengths) if k != longest)     # the longest frame gets no lanes

    def plan(sub):
        want = [_rounds(data, head, sub) for data, head in frames]
        most = min(r for k, r in enumerate(want) if k != longest)
        return most, [(-1 if k == longest or r > most else r) for k, r in enumerate(want)]
    sub = max(SUBS[:2], key=lambda s: len(set(plan(s)[1])))
    max_rounds, expect = plan(sub)
    assert -1 in expect and max(expect) >= 1
    batch, expect = frames + frames[::-1], expect + expect[::-1]
    runs = [_abi_run(gpu, batch, sub, max_rounds, max_scan, fill=fill) for _ in range(2)]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs))
    pixels, status, rounds = runs[0]
    n = len(batch)
    assert all((x[-64:] == fill).all() for x in runs[0])
    assert rounds[:-64].view(np.int32).tolist() == expect and not status[:-64].any()
    assert np.array_equal(pixels[:-64], np.concatenate([_decoded(d, hd)[0].ravel() for d, hd in batch]))
    # chunks: a workspace of 3 frames for a batch of 6
    head = batch[0][1]
    size = lambda k: int(gpu.va_jpeg_decode_split_workspace_bytes(k, head["h"], head["w"], head["c"],
                                                                   head["sampling"][0], head["sampling"][1], sub, max_scan))
    assert n == 6 and 2 * size(3) < size(6) + 4096
    chunked = _abi_run(gpu, batch, sub, max_rounds, max_scan, workspace_bytes=size(3), fill=fill ^ 0xFF)
    assert all(np.array_equal(a[:-64], b[:-64]) for a, b in zip(chunked, runs[0]))
    from video import _hip
    with pytest.raises(_hip.HipError) as err:
        _abi_run(gpu, batch, sub, max_rounds, max_scan, workspace_bytes=size(1) - 256)
    assert err.value.code == -34 and "one frame" in str(err.value)
    # hostile streams between valid neighbours
    for key in ("420", "mono"):
        items = hostile[key]
        good = items[0]
        group = [(d, hd) for _, d, hd in [good] + items[1:] + [good]]
        most = max(_segment(d, hd).lanes(sub) for d, hd in group)
        longest = max(len(d) - hd["scan_begin"] for d, hd in group)
        pixels, status, rounds = _abi_run(gpu, group, sub, most, longest, fill=fill)
        assert (pixels[-64:] == fill).all() and (status[-64:] == fill).all() and (rounds[-64:] == fill).all()
        want = [_decoded(d, hd) for d, hd in group]
        assert status[:-64].view(np.int32).tolist() == [st for _, st in want]
        assert np.array_equal(pixels[:-64], np.concatenate([px.ravel() for px, _ in want]))
        assert rounds[:-64].view(np.int32).tolist() == [_rounds(d, hd, sub) for d, hd in group]
        assert len({st for _, st in want}) >= 3


def test_raw_abi_mixed_batches_hostile_streams_chunks_and_two_runs(gpu, valid, hostile):
    _check_abi(gpu, valid, hostile, 0xA5)


def test_a_dc_value_out_of_range_in_a_late_subsequence(gpu, hostile, valid, monkeypatch):
    """the scan sees nothing, the write pass finds it, the seal zeroes the lanes behind it; next to valid frames"""
    (name, data, head), = hostile["dc"]
    good = [it for it in valid["mono"] if it[0].startswith("64x48")][:2]
    assert _decoded(data, head)[1] == D.BAD_CODE and all(it[2]["qtables"].tobytes() == head["qtables"].tobytes() for it in good)
    for sub in SUBS:
        batch = [good[0], (name, data, head), good[1]]
        most = max(_segment(d, hd).lanes(sub) for _, d, hd in batch)
        assert _check_batch(batch, sub, most, monkeypatch) == 0


def test_on_filled_memory_with_guarded_tails(gpu, valid, hostile, monkeypatch):
    """the ABI runs and one ops.jpeg_decode batch per layout with the test fill mode on: undefined device memory holds
    the fill byte and every buffer has a guarded tail ("Hostile memory")"""
    from video import _hip, ops
    ops.pool_clear()
    _hip.set_fill_mode(0xFF)
    try:
        _check_abi(gpu, valid, hostile, 0xFF)
        for layout in P.LAYOUTS:
            batch = _by_shape(valid[layout])[-1]
            most = max(_segment(d, hd).lanes(48) for _, d, hd in batch)
            assert _check_batch(batch, 48, most, monkeypatch) == 0
            assert _check_batch(batch, 48, 1, monkeypatch) >= 0
        found = _hip.check_guards()
    finally:
        _hip.set_fill_mode(-1)
        ops.pool_clear()
        _hip.check_guards()
    assert found == [], found


@pytest.fixture(scope="module")
def pictures():
    """256 x 256 frames without restart markers, smooth and noisy, and what the restatements say of them:
    [(name, data, head)]"""
    out = []
    for layout, sigma, quality in (("420", 2.0, 90), ("420", 20.0, 50), ("mono", 20.0, 90), ("444", 2.0, 50)):
        data = P.encode_plain(P.picture(256, 256, 31, sigma), layout, quality)
        out.append(("%s sigma %g q%d" % (layout, sigma, quality), data, D.parse_header(data, sampling="any")))
    return out


def test_default_routing_and_default_conditions(gpu, pictures):
    """through the defaults (split=None) a 256 x 256 frame without restart markers is split (rounds >= 1: on the
    one-lane path it would be 0), a frame with a restart interval per MCU row is not; with the default sub_bytes and
    max_rounds none of the pictures falls back, as the restated scan says beforehand"""
    from video import ops
    for name, data, head in pictures:
        want = _rounds(data, head, ops.JPEG_SPLIT_SUB_BYTES)
        assert 1 <= want <= ops.JPEG_SPLIT_MAX_ROUNDS, (name, want)
        assert len(data) - head["scan_begin"] >= ops.JPEG_SPLIT_MIN_BYTES, name
        got, status, rounds = ops.jpeg_decode([data, data], ret_status=True, ret_rounds=True)
        pixels, want_status = _decoded(data, head)
        assert rounds.tolist() == [want, want] and status.tolist() == [want_status, want_status] == [0, 0], name
        assert np.array_equal(got[0], pixels) and np.array_equal(got[1], pixels), name
        assert np.array_equal(ops.jpeg_decode([data], split=False), got[:1]), name
    rows = S.encode_frame(P.picture(256, 256, 31, 2.0), 90, (2, 2))
    assert D.parse_header(rows, sampling="any")["nseg"] == 16
    got, rounds = ops.jpeg_decode([rows], ret_rounds=True)
    assert rounds.tolist() == [0] and np.array_equal(got[0], S.decode(rows)[0])
