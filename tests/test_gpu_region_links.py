"""GPU: va_region_links, ops.region_links, FrameEngine's 'links' output and track_regions against the NumPy
restatement of tests/region_links_checks.py ("Region links").  Every comparison is of bytes.  The raw
calls run on buffers that were filled with a pattern first, links, counts and totals each with a tail behind them, so
that a write beyond a capacity or a buffer shows; the `hostile` fixture (the pattern of tests/test_gpu_hostile_memory.py)
repeats the op and engine tests on dirty pooled memory with guarded tails."""
import numpy as np
import pytest

import region_links_checks as K

pytestmark = pytest.mark.gpu

TAIL = 256
FILLS = (0xFF, 0xA5)


@pytest.fixture(params=FILLS, ids=["fill_ff", "fill_a5"])
def hostile(request):
    """the test fill mode, on around one test; no guarded buffer leaks into another module's tests and no unguarded
    one into these"""
    from video import _hip, ops
    _hip.lib()
    ops.pool_clear()
    _hip.set_fill_mode(request.param)
    try:
        yield request.param
        found = _hip.check_guards()
    finally:
        _hip.set_fill_mode(-1)
        ops.pool_clear()
        _hip.check_guards()             # (what pool_clear's free() may still have recorded is not a later test's)
    assert found == [], found


def _filled(nbytes, byte):
    from video import _hip
    buf = _hip.DeviceBuffer(nbytes + TAIL)
    _hip.check(_hip.lib().va_memset(buf.ptr, byte, nbytes + TAIL, None))
    return buf


def abi(labels, prev=None, cap=None, pattern=0xA5, null_links=False):
    """one va_region_links call on patterned buffers with tails.  Returns total, need, per (n,), rows (the first
    min(total, cap) records), and `clean`: every byte behind the records written, behind the counts and behind the
    totals still holds the pattern"""
    from video import _hip
    L = _hip.lib()
    labels = np.ascontiguousarray(labels, np.int32)
    n, h, w = labels.shape
    cap = K.need_of(labels, prev) if cap is None else cap
    ws_bytes = L.va_region_links_workspace_bytes(n, h, w, cap)
    lab = _hip.DeviceBuffer.from_array(labels) if labels.size else _hip.DeviceBuffer(4)
    pv = None if prev is None else _hip.DeviceBuffer.from_array(np.ascontiguousarray(prev, np.int32))
    rec, nl, tot, ws = _filled(cap * 16, pattern), _filled(n * 4, pattern), _filled(16, pattern), _filled(ws_bytes, pattern)
    try:
        _hip.check(L.va_region_links(None if pv is None else pv.ptr, lab.ptr, n, h, w, nl.ptr, tot.ptr,
                                     None if null_links else rec.ptr, cap, ws.ptr, ws_bytes, None))
        _hip.check(L.va_stream_sync(None))
        raw = rec.download((cap * 16 + TAIL,), np.uint8)
        per = nl.download((n * 4 + TAIL,), np.uint8)
        totals = tot.download((16 + TAIL,), np.uint8)
    finally:
        for b in (lab, pv, rec, nl, tot, ws):
            if b is not None:
                b.free()
    total, need = (int(v) for v in totals[:16].view(np.int64))
    stored = total if need <= cap else 0
    clean = bool((raw[stored * 16:] == pattern).all() and (per[n * 4:] == pattern).all()
                 and (totals[16:] == pattern).all())
    return dict(total=total, need=need, per=per[:n * 4].view(np.int32).copy(), clean=clean, stored=stored,
                rows=raw[:stored * 16].view(np.int32).reshape(-1, 4).copy())


def check_case(name, labels, prev):
    """the raw call with cap = need and ops.region_links, both against the restatement"""
    from video import ops
    want, per = K.restate(labels, prev)
    need = K.need_of(labels, prev)
    got = abi(labels, prev)
    assert (got["total"], got["need"]) == (len(want), need), name
    assert np.array_equal(got["rows"], want) and np.array_equal(got["per"], per) and got["clean"], name
    links = ops.region_links(labels, prev)
    assert links.offsets.dtype == np.int64 and links.a.dtype == links.b.dtype == links.count.dtype == np.int32, name
    assert np.array_equal(K.as_rows(links), want), name
    assert np.array_equal(np.diff(links.offsets), per) and links.offsets[0] == 0, name


# ------------------------------------------------------------------------------------------------ shapes and contents
@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: "%dx%d" % s)
def test_frame_shapes_and_counts(shape):
    ran = 0
    for name, (labels, prev) in K.shape_cases().items():
        if labels.shape[1:] == shape:
            check_case(name, labels, prev)
            ran += 1
    assert ran == 2 * len(K.COUNTS)


@pytest.mark.parametrize("name", sorted(K.content_cases()))
def test_label_contents(name):
    labels, prev = K.content_cases()[name]
    check_case(name, labels, prev)
    want, _ = K.restate(labels, prev)
    if name == "background":
        assert len(want) == 0
    if name == "one_label":
        assert want.tolist() == [[0, 3, 7, 37 * 53], [1, 7, 7, 37 * 53]]
    if name == "stripes":
        assert len(want) == 4 * 37 * 53
    if name == "giant_vs_500_singles":
        assert np.bincount(want[:, 0]).tolist() == [500, 500, 500]
    if name == "wide_labels":
        assert want[:, 1:3].max() == K.I32_MAX
    if name == "empty_pairs_between":
        assert np.bincount(want[:, 0], minlength=5).tolist() == [3, 9, 0, 0, 9]


def check_fixture_cases():
    for name, (labels, prev, want) in K.fixture().items():
        got = abi(labels, prev)
        assert np.array_equal(got["rows"], want) and got["clean"], name


def test_fixture_cases():
    check_fixture_cases()


def test_no_frames():
    from video import ops
    got = abi(np.zeros((0, 4, 5), np.int32), cap=3)
    assert (got["total"], got["need"], got["clean"]) == (0, 0, True)
    links = ops.region_links(np.zeros((0, 4, 5), np.int32), prev=np.ones((4, 5), np.int32))
    assert links.offsets.tolist() == [0] and links.a.size == links.b.size == links.count.size == 0


def test_arguments():
    from video import _hip, ops
    L = _hip.lib()
    buf = _hip.DeviceBuffer(8192)
    _hip.check(L.va_memset(buf.ptr, 0, 8192, None))
    ws = L.va_region_links_workspace_bytes(1, 4, 4, 8)
    call = lambda **k: L.va_region_links(*[k.get(name, default) for name, default in (
        ("prev", None), ("labels", buf.ptr), ("n", 1), ("h", 4), ("w", 4), ("nlinks", buf.ptr + 256),
        ("totals", buf.ptr + 512), ("links", buf.ptr + 768), ("cap", 0), ("ws", buf.ptr + 1024), ("ws_bytes", ws),
        ("stream", None))])
    try:
        assert L.va_region_links_workspace_bytes(1, 4, 4, 0) <= ws <= 7168 and call() == 0 and call(cap=8) == 0
        for bad in (dict(n=-1), dict(h=0), dict(w=-3), dict(cap=-1), dict(labels=None), dict(nlinks=None),
                    dict(totals=None), dict(ws=None), dict(links=None, cap=8), dict(ws_bytes=ws - 1, cap=8),
                    dict(h=1 << 15, w=1 << 14)):
            assert call(**bad) == -22, bad                           # VA_ERR_INVALID
        _hip.check(L.va_stream_sync(None))
    finally:
        buf.free()
    with pytest.raises(ValueError):
        ops.region_links(np.zeros((4, 4), np.int32))
    with pytest.raises(ValueError):
        ops.region_links(np.zeros((2, 4, 4), np.int32), prev=np.zeros((4, 5), np.int32))


# ------------------------------------------------------------------------------------------------ capacity
CAPACITY_CASES = ("shifted", "giant_vs_500_singles", "wide_labels", "stripes")


def check_capacity(name):
    """cap = need - 1, need, 0 and need + 1000.  Below need nothing is stored, and the links per pair and both totals
    are still the true numbers.  With these capacities the tables of giant_vs_500_singles fit the workspace together
    (the pairs are counted side by side); those of shifted, wide_labels and stripes (need above the pixels of a
    frame) do not, and are counted a table at a time."""
    labels, prev = K.content_cases()[name]
    want, per = K.restate(labels, prev)
    need = K.need_of(labels, prev)
    assert len(want) <= need and (name != "shifted" or len(want) < need)
    for cap, null_links in ((need - 1, False), (0, False), (0, True)):
        short = abi(labels, prev, cap=cap, null_links=null_links)
        assert short["clean"] and short["stored"] == 0, (name, cap)       # the records and their tail are untouched
        assert (short["total"], short["need"]) == (len(want), need), (name, cap)
        assert np.array_equal(short["per"], per), (name, cap)
    exact = abi(labels, prev, cap=need)
    assert exact["clean"] and (exact["total"], exact["need"]) == (len(want), need) and np.array_equal(exact["rows"], want)
    roomy = abi(labels, prev, cap=need + 1000)
    assert roomy["clean"] and roomy["stored"] == len(want) and np.array_equal(roomy["rows"], want)
    assert np.array_equal(roomy["per"], per) and (roomy["total"], roomy["need"]) == (len(want), need)


@pytest.mark.parametrize("name", CAPACITY_CASES)
def test_capacity(name):
    check_capacity(name)


def _counting(monkeypatch):
    from video import _hip
    real = _hip.lib()

    class Counting(object):
        """the library with its va_region_links calls counted: the capacity of each"""
        caps = []

        def __getattr__(self, name):
            fn = getattr(real, name)
            if name != "va_region_links":
                return fn

            def counted(*args):
                self.caps.append(args[8])
                return fn(*args)
            return counted
    proxy = Counting()
    monkeypatch.setattr(_hip, "lib", lambda device=None: proxy)
    return proxy


def test_retry_through_ops(monkeypatch):
    from video import ops
    labels, prev = K.content_cases()["stripes"]
    want, _ = K.restate(labels, prev)
    need = K.need_of(labels, prev)
    proxy = _counting(monkeypatch)
    assert np.array_equal(K.as_rows(ops.region_links(labels, prev)), want)
    assert proxy.caps == [ops.DEFAULT_LINK_CAPACITY] and need <= ops.DEFAULT_LINK_CAPACITY     # room: one launch
    del proxy.caps[:]
    assert np.array_equal(K.as_rows(ops.region_links(labels, prev, cap=10)), want)
    assert proxy.caps == [10, need]                                                            # exactly one more
    del proxy.caps[:]
    assert np.array_equal(K.as_rows(ops.region_links(labels, prev, cap=0)), want) and proxy.caps == [0, need]
    del proxy.caps[:]
    assert np.array_equal(K.as_rows(ops.region_links(labels, prev, cap=need)), want) and proxy.caps == [need]


# ------------------------------------------------------------------------------------------------ grid and load
def restate_tiny(labels, prev):
    """the restatement for many pairs of few pixels, vectorised over the pairs"""
    n = len(labels)
    L = labels.reshape(n, -1).astype(np.int64)
    E = np.concatenate([prev.reshape(1, -1), L[:-1]]).astype(np.int64)
    key = np.where((E >= 1) & (L >= 1), (E << 32) | L, 0)
    px = key.shape[1]
    same = key[:, :, None] == key[:, None, :]                      # (n, i, j)
    earlier = np.tril(np.ones((px, px), bool), -1)[None]           # j < i
    first = (key != 0) & ~(same & earlier).any(2)
    t, i = np.nonzero(first)
    k = key[t, i]
    return np.stack([t, k >> 32, k & 0xffffffff, same.sum(2)[t, i]], 1).astype(np.int32)


@pytest.fixture(scope="module")
def many_pairs():
    rng = np.random.default_rng(70)
    labels = rng.integers(-1, 3, (70000, 2, 2)).astype(np.int32)
    prev = rng.integers(-1, 3, (2, 2)).astype(np.int32)
    want = restate_tiny(labels, prev)
    assert np.array_equal(want[want[:, 0] < 50], K.restate(labels[:50], prev)[0]) and want[-1, 0] > 69990
    return labels, prev, want


@pytest.fixture(scope="module")
def noise_pair():
    """two 1080p frames of 50 % noise, labelled on the device: about 10^5 regions each"""
    from video import _hip, ops
    assert _hip.fill_mode() == -1
    masks = (np.random.default_rng(1080).random((2, 1080, 1920)) < 0.5).astype(np.uint8)
    labels, counts = ops.label(masks, connectivity=4)
    assert counts.min() > 50000
    want, _ = K.restate(labels, labels[1])
    assert len(want) > 100000
    return labels, labels[1], want


def test_70000_pairs(many_pairs):
    from video import ops
    labels, prev, want = many_pairs
    assert np.array_equal(K.as_rows(ops.region_links(labels, prev, cap=len(want) + 7)), want)


def test_1080p_noise_labels_and_determinism(noise_pair):
    labels, prev, want = noise_pair
    need = K.need_of(labels, prev)
    one, two = abi(labels, prev, cap=need, pattern=0xA5), abi(labels, prev, cap=need + 4096, pattern=0xFF)
    assert one["clean"] and two["clean"]
    assert np.array_equal(one["rows"], want) and (one["total"], one["need"]) == (len(want), need)
    assert one["rows"].tobytes() == two["rows"].tobytes() and one["per"].tobytes() == two["per"].tobytes()
    assert (one["total"], one["need"]) == (two["total"], two["need"])


def test_short_capacity_counts_exactly_under_load(many_pairs, noise_pair):
    """cap = 0 on the two loads: the tables do not fit together, every pair is counted with a table at a time"""
    for labels, prev, want in (many_pairs, noise_pair):
        got = abi(labels, prev, cap=0)
        assert got["clean"] and got["stored"] == 0
        assert (got["total"], got["need"]) == (len(want), K.need_of(labels, prev))
        assert np.array_equal(got["per"], np.bincount(want[:, 0], minlength=len(labels)))


def check_1080p_blob_pair():
    from video import ops
    yy, xx = np.mgrid[:1080, :1920]
    labels = np.zeros((2, 1080, 1920), np.int32)
    for t in range(2):
        for k, (cx, cy, r) in enumerate(((300, 200, 150), (900, 540, 300), (1500, 800, 220), (1000, 500, 40))):
            labels[t][(xx - cx - 60 * t) ** 2 + (yy - cy + 25 * t) ** 2 <= r * r] = k + 1
    want, _ = K.restate(labels, labels[1])
    assert 6 <= len(want) <= 16
    assert np.array_equal(K.as_rows(ops.region_links(labels, labels[1])), want)


def test_1080p_blob_pair():
    check_1080p_blob_pair()


# ------------------------------------------------------------------------------------------------ hostile memory
def test_hostile_capacity_fixture_and_blobs(hostile):
    for name in CAPACITY_CASES:
        check_capacity(name)
    check_fixture_cases()
    check_1080p_blob_pair()


def test_hostile_small_cases(hostile):
    from video import ops
    for cases in (K.shape_cases(), K.content_cases()):
        for name, (labels, prev) in cases.items():
            want, _ = K.restate(labels, prev)
            for again in range(2):
                assert np.array_equal(K.as_rows(ops.region_links(labels, prev, cap=(None, 3)[again])), want), name


def test_hostile_grid_and_load(hostile, many_pairs, noise_pair):
    from video import ops
    for labels, prev, want in (many_pairs, noise_pair):
        for again in range(2):
            assert np.array_equal(K.as_rows(ops.region_links(labels, prev)), want)


# ------------------------------------------------------------------------------------------------ the engine
H, W = 48, 64


def _engine(max_batch=12):
    from video.engine import FrameEngine
    return FrameEngine(size=(W, H), max_batch=max_batch, thresh=100, connectivity=8, max_labels=8)


@pytest.fixture(scope="module")
def clip():
    """the clip, its labels and counts from a plain run, and the restatement's links on them"""
    from video import _hip
    assert _hip.fill_mode() == -1
    frames = K.blob_clip(12, H, W)
    eng = _engine()
    try:
        plain = eng.run(frames, want=("mask", "labels", "counts"))
    finally:
        eng.close()
    want, _ = K.restate(plain["labels"])
    assert plain["counts"].min() >= 3 and len(set(plain["counts"].tolist())) >= 2 and len(want) >= 30
    return frames, plain, want


def _joined(parts):
    """the rows of consecutive runs, the frames numbered through"""
    rows, first = [], 0
    for links in parts:
        r = K.as_rows(links)
        r[:, 0] += first
        rows.append(r)
        first += len(links.offsets) - 1
    return np.concatenate(rows)


def check_engine(clip, monkeypatch):
    from video import _hip, ops
    frames, plain, want = clip
    eng = _engine()
    try:
        whole = eng.run(frames, want=("counts", "stats", "links"))
        assert sorted(whole) == ["counts", "links", "stats"] and np.array_equal(whole["counts"], plain["counts"])
        assert np.array_equal(K.as_rows(whole["links"]), want)
        # a second video: without reset_links frame 0 links to the last frame of the run before
        again = eng.run(frames, want=("links",))
        assert sorted(again) == ["links"]
        bridge = K.pair_links(plain["labels"][11], plain["labels"][0])
        assert len(bridge) and np.array_equal(K.as_rows(again["links"]), K.restate(plain["labels"], plain["labels"][11])[0])
        eng.reset_links()
        parts = [eng.run(frames[:5], want=("links", "counts"))["links"]]
        # a run without 'links' returns what it returned before, and leaves the kept plane as it is
        other = eng.run(frames[6:9], want=("mask", "labels", "counts"))
        assert sorted(other) == ["counts", "labels", "mask"]
        for key in other:
            assert np.array_equal(other[key], plain[key][6:9]), key
        parts.append(eng.run(frames[5:], want=("links",))["links"])
        assert np.array_equal(_joined(parts), want)
        # frames that are on the device already; no download of a plane
        eng.reset_links()
        sizes, real = [], _hip.DeviceBuffer.download
        dev = ops.DeviceFrames.upload(frames)
        with monkeypatch.context() as patch:
            patch.setattr(_hip.DeviceBuffer, "download",
                          lambda self, shape, dtype, stream=None: sizes.append(int(np.prod(shape))) or real(self, shape, dtype, stream))
            try:
                resident = eng.run_frames(dev, want=("counts", "stats", "links"))
            finally:
                dev.release()
        assert np.array_equal(K.as_rows(resident["links"]), want) and np.array_equal(resident["stats"], whole["stats"])
        assert sizes and max(sizes) < H * W, sizes
        with pytest.raises(ValueError):
            eng._check_keep(("labels",))
        with pytest.raises(ValueError):
            eng.run(frames, want=("links", "tracks"))
    finally:
        eng.close()


def test_engine_links(clip, monkeypatch):
    check_engine(clip, monkeypatch)


def test_engine_links_hostile(clip, hostile, monkeypatch):
    check_engine(clip, monkeypatch)


def test_engine_without_labelling_has_no_links():
    from video.engine import FrameEngine
    eng = FrameEngine(size=(W, H), max_batch=2, thresh=100)
    try:
        with pytest.raises(ValueError):
            eng.run(np.zeros((2, H, W), np.uint8), want=("links",))
    finally:
        eng.close()


def test_track_regions(clip):
    check_track_regions(clip)


def test_track_regions_hostile(clip, hostile):
    check_track_regions(clip)


def check_track_regions(clip):
    from video import ops
    from video.analysis.tracking import RegionTracker, track_regions
    frames, plain, want = clip
    offsets = np.concatenate([[0], np.cumsum(np.bincount(want[:, 0], minlength=12))])
    ids, lin, lout = RegionTracker().update((offsets, want[:, 1], want[:, 2], want[:, 3]), plain["counts"])
    assert max(i.max() for i in ids) + 1 > plain["counts"].max()        # regions are born along the way
    assert any((v >= 2).any() for v in lin) or any((v >= 2).any() for v in lout)
    eng = _engine(max_batch=5)
    try:
        for source in (frames, ops.DeviceFrames.upload(frames)):
            try:
                got = track_regions(eng, source, batch=5)
            finally:
                if source is not frames:
                    source.release()
            assert np.array_equal(got.counts, plain["counts"]) and len(got.stats) == 12
            for t in range(12):
                assert np.array_equal(got.ids[t], ids[t]) and got.ids[t].dtype == np.int64, t
                assert np.array_equal(got.links_in[t], lin[t]) and np.array_equal(got.links_out[t], lout[t]), t
                assert got.stats[t].shape == (plain["counts"][t], 16)
    finally:
        eng.close()
