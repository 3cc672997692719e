"""GPU: va_template_match_u8, ops.match_templates, image.match_template / find_template and TemplateTracker (DESIGN.md
§9, "Template matching") against the fixture two restatements agreed on and against the restatements themselves.  Every
comparison is of bytes: the best records, the score maps and the statuses, for all six methods.  The raw calls run on
pattern-filled outputs and a workspace with tails behind them, and a flagged query must leave all of its record but the
status as the pattern; the `hostile` fixture (the pattern of tests/test_gpu_sliding_median.py, fill bytes 0x00 and
0xFF) repeats the fixture on dirty pooled memory with guarded tails."""
import ctypes as C
import time

import numpy as np
import pytest

import template_match_checks as K

pytestmark = pytest.mark.gpu

TAIL = 256
FILLS = (0x00, 0xFF)


@pytest.fixture(scope="module")
def cases():
    return K.fixture()


@pytest.fixture(params=FILLS, ids=["fill_00", "fill_ff"])
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


class Buffers(object):
    """the device buffers of raw calls on one set of inputs.  Frames and templates are entered `late` bytes into their
    buffers, every typed array `late` elements; the frames lie `stride` bytes apart.  Outputs and the workspace are
    filled with `pattern` and have a tail behind them."""

    def __init__(self, frames, templates, queries, stride=None, late=0, pattern=0xA5, total=None, shapes=None):
        from video import _hip
        self.L = _hip.lib()
        n, h, w = frames.shape
        self.n, self.h, self.w, self.late, self.pattern = n, h, w, late, pattern
        self.stride = h * w if stride is None else stride
        self.queries = np.ascontiguousarray(queries, np.int32).reshape(-1, 6)
        self.nq, self.m = len(self.queries), len(templates)
        tbytes, real_shapes, offsets = K.pack_templates(templates)
        status = np.array([K.status_of(q, n, h, w, [t.shape for t in templates]) for q in self.queries], np.int32)
        self.map_off = K.map_offsets(self.queries, status) if self.nq else np.zeros(1, np.int64)
        self.true_total = int(self.map_off[-1])
        self.total = self.true_total if total is None else total
        self.ws_bytes = self.L.va_template_match_workspace_bytes(self.nq, self.total, self.m)
        self.frame_bytes = (n - 1) * self.stride + h * w if n else 0
        self.inputs = dict(frames=(self.flat_frames(frames), late), templates=(tbytes, late),
                           shapes=(real_shapes if shapes is None else np.asarray(shapes, np.int32), 4 * late),
                           offsets=(offsets, 8 * late), queries=(self.queries, 4 * late), map_off=(self.map_off, 8 * late))
        self.dev, self.at = {}, {}
        for name, (arr, skip) in self.inputs.items():
            self.dev[name] = _hip.DeviceBuffer(skip + arr.nbytes + 1)
            self.at[name] = self.dev[name].ptr + skip
            self.load(name, arr)
        self.out_bytes = dict(best=self.nq * 24, maps=self.true_total * 8, ws=self.ws_bytes)
        for name, nbytes in self.out_bytes.items():
            self.dev[name] = _hip.DeviceBuffer(8 * late + nbytes + TAIL)
            self.at[name] = self.dev[name].ptr + 8 * late
        self.reset()

    def flat_frames(self, frames):
        flat = np.full(self.frame_bytes, 0x5A, np.uint8)
        for i in range(self.n):
            flat[i * self.stride:i * self.stride + self.h * self.w] = frames[i].reshape(-1)
        return flat

    def load(self, name, arr):
        from video import _hip
        arr = np.ascontiguousarray(arr)
        if arr.nbytes:
            _hip.check(self.L.va_memcpy_h2d(self.at[name], arr.ctypes.data, arr.nbytes, None))
            _hip.check(self.L.va_stream_sync(None))

    def reset(self):
        from video import _hip
        for name in self.out_bytes:
            _hip.check(self.L.va_memset(self.dev[name].ptr, self.pattern, self.dev[name].nbytes, None))
        _hip.check(self.L.va_stream_sync(None))

    def call(self, method, maps=True, best=True, stream=None, **changes):
        from video import _hip
        fields = dict(struct_size=C.sizeof(_hip.va_match_args), method=K.METHODS.index(method),
                      frames_dev=self.at["frames"], n=self.n, h=self.h, w=self.w, reserved=0, frame_stride=self.stride,
                      templates_dev=self.at["templates"], template_shapes_dev=self.at["shapes"],
                      template_offsets_dev=self.at["offsets"], n_templates=self.m, queries_dev=self.at["queries"],
                      n_queries=self.nq, total_positions=self.total, best_out_dev=self.at["best"] if best else None,
                      maps_out_dev=self.at["maps"] if maps else None, map_offsets_dev=self.at["map_off"] if maps else None,
                      workspace_dev=self.at["ws"], workspace_bytes=self.ws_bytes, stream=getattr(stream, "value", stream))
        fields.update(changes)
        return self.L.va_template_match_u8(C.byref(_hip.va_match_args(**fields)))

    def outputs(self, stream=None):
        """(best BEST_DTYPE (q,), maps flat float64, clean): clean says that what lies in front of and behind the
        outputs and the workspace still holds the pattern"""
        from video import _hip
        _hip.check(self.L.va_stream_sync(stream))
        raw = {name: self.dev[name].download((self.dev[name].nbytes,), np.uint8) for name in self.out_bytes}
        skip, clean = 8 * self.late, True
        for name, nbytes in self.out_bytes.items():
            clean = clean and bool((raw[name][:skip] == self.pattern).all() and (raw[name][skip + nbytes:] == self.pattern).all())
        best = raw["best"][skip:skip + self.nq * 24].view(K.BEST_DTYPE)
        return best, raw["maps"][skip:skip + self.true_total * 8].view(np.float64), clean

    def free(self):
        for buf in self.dev.values():
            buf.free()


def expected(want, pattern=0xA5):
    """the bytes a call leaves in pattern-filled outputs: want = (best, maps) of K.restate.  A flagged query writes its
    status and nothing else"""
    best, maps = want
    out = np.full(len(best) * 24, pattern, np.uint8).view(K.BEST_DTYPE).copy()
    good = best["status"] == 0
    out[good] = best[good]
    out["status"][~good] = best["status"][~good]
    flat = [m.reshape(-1) for m in maps if m is not None]
    return out, np.concatenate(flat) if flat else np.zeros(0)


def run_raw(frames, templates, queries, method, **layout):
    """one raw call with both outputs: (rc, best, maps flat, clean)"""
    maps, best = layout.pop("maps", True), layout.pop("best", True)
    bufs = Buffers(frames, templates, queries, **layout)
    try:
        rc = bufs.call(method, maps=maps, best=best)
        return (rc,) + bufs.outputs()
    finally:
        bufs.free()


def check_raw(frames, templates, queries, methods=K.METHODS, want=None, **layout):
    pattern = layout.get("pattern", 0xA5)
    for method in methods:
        rc, best, maps, clean = run_raw(frames, templates, queries, method, **layout)
        truth = want[method] if want else K.restate(frames, templates, queries, method)
        want_best, want_maps = expected(truth, pattern)
        assert rc == 0 and clean, (method, rc)
        assert best.tobytes() == want_best.tobytes(), (method, best, want_best)
        assert maps.tobytes() == want_maps.tobytes(), (method, int(np.count_nonzero(maps != want_maps)))


# ------------------------------------------------------------------------------------------------ the fixture
@pytest.mark.parametrize("layout", (dict(), dict(late=1, stride=48 * 83 + 5, pattern=0x00),
                                    dict(late=3, stride=48 * 83 + 4, pattern=0xFF)), ids=("plain", "late_1", "late_3"))
def test_fixture_raw_all_methods(cases, layout):
    """every template shape, window placement, zero denominator and bad query of the fixture; frames and templates
    entered 1 and 3 bytes late, with a frame stride larger than h * w"""
    frames, templates, queries, want = cases
    check_raw(frames, templates, queries, want=want, **layout)


def test_each_output_alone(cases):
    frames, templates, queries, want = cases
    want_best, want_maps = expected(want["ccoeff"])
    rc, best, maps, clean = run_raw(frames, templates, queries, "ccoeff", maps=False)
    assert rc == 0 and clean and best.tobytes() == want_best.tobytes() and (maps.view(np.uint8) == 0xA5).all()
    rc, best, maps, clean = run_raw(frames, templates, queries, "ccoeff", best=False)
    assert rc == 0 and clean and maps.tobytes() == want_maps.tobytes() and (best.view(np.uint8) == 0xA5).all()


def check_fixture_through_ops(cases, methods=K.METHODS):
    from video import ops
    frames, templates, queries, want = cases
    dev = ops.DeviceFrames.upload(frames)
    try:
        for k, method in enumerate(methods):
            best, maps = ops.match_templates(dev if k % 2 else frames, templates, queries, method=method, maps=True)
            truth, truth_maps = want[method]
            good = truth["status"] == 0
            assert best.dtype == ops.MATCH_RESULT_DTYPE and np.array_equal(best["status"], truth["status"])
            for name in ("score", "x", "y"):
                assert best[name][good].tobytes() == truth[name][good].tobytes(), (method, name)
            assert np.isnan(best["score"][~good]).all() and (best["x"][~good] == -1).all() and (best["y"][~good] == -1).all()
            for got, wanted in zip(maps, truth_maps):
                assert got.tobytes() == wanted.tobytes() if wanted is not None else got.shape == (0, 0), method
            alone = ops.match_templates(frames, templates, queries, method=method)
            assert alone.tobytes() == best.tobytes(), method
        assert np.array_equal(dev.download(), frames)
    finally:
        dev.release()


def test_fixture_through_ops(cases):
    check_fixture_through_ops(cases)


def test_fixture_through_ops_on_hostile_memory(cases, hostile):
    check_fixture_through_ops(cases)


# ------------------------------------------------------------------------------------------------ shapes the fixture has no room for
def test_template_of_255s_fills_32_bits():
    """256 x 256 of 255 on 257 x 258 of 255: S_it = 4 261 478 400 > 2^31; a signed or narrowed accumulator fails it"""
    frames = np.full((1, 257, 258), 255, np.uint8)
    templates = [np.full((256, 256), 255, np.uint8)]
    queries = [(0, 0, 0, 0, 3, 2)]
    best, _ = K.restate(frames, templates, queries, "ccorr")
    assert best["score"][0] == 4261478400.0
    check_raw(frames, templates, queries)
    frames[0, 100:, 7:] = 254                          # ... and with the sums apart from one another
    check_raw(frames, templates, queries)


def test_templates_beyond_one_chunk_and_windows_at_the_tile_size():
    """templates taller than the row chunk, wider than the column chunk and both, with columns that are no multiple
    of four; windows of one tile less one, one tile and one tile more one each way"""
    rng = np.random.default_rng(41)
    frames = rng.integers(0, 256, (2, 121, 271), dtype=np.uint8)
    shapes = ((5, 7), (3, 4), (K.CHUNK_ROWS + 24, 3), (3, 3 * K.CHUNK_COLS + 9), (2 * K.CHUNK_ROWS + 6, 2 * K.CHUNK_COLS + 2),
              (K.CHUNK_ROWS, K.CHUNK_COLS), (K.CHUNK_ROWS + 1, K.CHUNK_COLS + 1))
    templates = [rng.integers(0, 256, s, dtype=np.uint8) for s in shapes]
    frames[1, 50:50 + 38, 100:100 + 130] = templates[4]
    sizes = (K.TILE - 1, K.TILE, K.TILE + 1)
    queries = [(k % 2, k % 2, 3 + k, 2 * k, nx, ny) for k, (nx, ny) in enumerate((a, b) for a in sizes for b in sizes)]
    queries += [(1, 2, 200, 60, 9, 5), (0, 3, 1, 100, 40, 3), (1, 4, 90, 40, 33, 33), (1, 4, 141, 83, 1, 1),
                (0, 5, 7, 9, 35, 6), (1, 6, 205, 104, 2, 1), (1, 0, 0, 0, 265, 117)]
    check_raw(frames, templates, np.array(queries, np.int32))
    check_raw(frames, templates, np.array(queries, np.int32), methods=("ccoeff_normed",), late=1, stride=121 * 271 + 7)


def test_ties_go_to_the_first_position_in_raster_order():
    constant = np.full((1, 50, 90), 131, np.uint8)
    templates = [np.full((3, 5), 77, np.uint8), np.array([[200, 0, 200], [0, 200, 0]], np.uint8)]
    window = (4, 2, 80, 45)                             # 3 x 2 tiles
    for method in K.METHODS:
        best, _ = K.restate(constant, templates, [(0, 0) + window, (0, 1) + window], method)
        assert best["x"].tolist() == [4, 4] and best["y"].tolist() == [2, 2], method
    check_raw(constant, templates, [(0, 0) + window, (0, 1) + window])
    planted = np.full((1, 50, 90), 9, np.uint8)         # two equal bests in different tiles: the earlier one wins
    planted[0, 40:42, 6:9] = planted[0, 5:7, 80:83] = templates[1]
    best, _ = K.restate(planted, templates, [(0, 1) + window], "ccoeff_normed")
    assert (best["x"][0], best["y"][0]) == (80, 5)
    check_raw(planted, templates, [(0, 1) + window])
    planted[0, 5:7, 80:83] = 9                          # ... in one tile row, the left one
    planted[0, 40:42, 70:73] = templates[1]
    best, _ = K.restate(planted, templates, [(0, 1) + window], "sqdiff")
    assert (best["x"][0], best["y"][0], best["score"][0]) == (6, 40, 0.0)
    check_raw(planted, templates, [(0, 1) + window])


def test_no_queries_and_seventy_thousand():
    from video import ops
    rng = np.random.default_rng(43)
    frames = rng.integers(0, 256, (50, 2, 2), dtype=np.uint8)
    templates = [np.array([[v]], np.uint8) for v in (0, 7, 255)]
    rc, best, maps, clean = run_raw(frames, templates, np.zeros((0, 6), np.int32), "ccorr")
    assert rc == 0 and clean and best.size == 0 and maps.size == 0
    nq = 70000                                          # more than gridDim.y / z hold
    queries = np.stack([rng.integers(0, 50, nq), rng.integers(0, 3, nq), rng.integers(0, 2, nq), rng.integers(0, 2, nq),
                        np.ones(nq, np.int64), np.ones(nq, np.int64)], axis=1).astype(np.int32)
    pixel = frames[queries[:, 0], queries[:, 3], queries[:, 2]].astype(np.int64)
    for method in ("sqdiff", "ccorr_normed", "sqdiff_normed"):
        want = np.zeros(nq)
        for t, templ in enumerate(templates):
            mine = queries[:, 1] == t
            want[mine] = K.score_map(method, templ, pixel[mine] * int(templ[0, 0]), pixel[mine], pixel[mine] ** 2)
        best, maps = ops.match_templates(frames, templates, queries, method=method, maps=True)
        assert not best["status"].any() and best["score"].tobytes() == want.tobytes(), method
        assert np.array_equal(best["x"], queries[:, 2]) and np.array_equal(best["y"], queries[:, 3])
        assert np.concatenate([m.reshape(-1) for m in maps]).tobytes() == want.tobytes()


def test_bad_templates_and_a_short_workspace_are_statuses():
    rng = np.random.default_rng(44)
    frames = rng.integers(0, 256, (1, 300, 300), dtype=np.uint8)
    templates = [rng.integers(0, 256, (4, 4), dtype=np.uint8), rng.integers(0, 256, (3, 5), dtype=np.uint8)]
    queries = np.array([(0, 0, 0, 0, 5, 5), (0, 1, 2, 2, 4, 3), (0, 0, 9, 9, 2, 2)], np.int32)
    truth = K.restate(frames, templates, queries, "ccoeff")
    for shapes, status in (([(4, 4), (0, 5)], K.BAD_SHAPE), ([(4, 4), (257, 256)], K.BAD_SHAPE), ([(4, 4), (4, 5)], K.BAD_SHAPE)):
        bufs = Buffers(frames, templates, queries, shapes=shapes)         # (4 x 5 does not fit between its offsets)
        try:
            assert bufs.call("ccoeff", maps=False) == 0
            best, _, clean = bufs.outputs()
        finally:
            bufs.free()
        want = expected(truth)[0]
        want[1] = np.full(24, 0xA5, np.uint8).view(K.BEST_DTYPE)[0]
        want["status"][1] = status
        assert clean and best.tobytes() == want.tobytes(), shapes
    # total_positions below what the queries need: the workspace has no room for the tiles; every query is flagged
    many = np.array([(0, 0, x, 0, K.TILE + 1, K.TILE + 1) for x in range(200)], np.int32)         # four tiles each
    bufs = Buffers(frames, templates, many, total=1)
    try:
        assert bufs.call("ccoeff", maps=False) == 0
        best, maps, clean = bufs.outputs()
    finally:
        bufs.free()
    want = np.full(200 * 24, 0xA5, np.uint8).view(K.BEST_DTYPE).copy()
    want["status"] = K.SHORT_WORKSPACE
    assert clean and best.tobytes() == want.tobytes() and (maps.view(np.uint8) == 0xA5).all()


def test_two_runs_write_identical_bytes(cases):
    frames, templates, queries, _ = cases
    bufs = Buffers(frames, templates, queries)
    try:
        runs = []
        for _ in range(2):
            bufs.reset()
            assert bufs.call("ccoeff_normed") == 0
            best, maps, clean = bufs.outputs()
            runs.append((best.tobytes(), maps.tobytes(), clean))
    finally:
        bufs.free()
    assert runs[0] == runs[1] and runs[0][2]


def test_stream_order_on_a_busy_stream(cases):
    """the call on a created stream that a blocker keeps busy: frames, templates and queries hold decoys until
    va_memcpy_d2d copies, enqueued on the same stream just before the call, deliver the true ones"""
    import pointer_offset_cases as P
    import stream_order_cases as S
    from video import _hip
    frames, templates, queries, want = cases
    queries = queries[want["ccoeff"][0]["status"] == 0]
    truth = expected(K.restate(frames, templates, queries, "ccoeff"))
    be = P.hip_backend()
    L = be.lib
    bufs = Buffers(frames, templates, queries)
    true_inputs = {name: np.ascontiguousarray(bufs.inputs[name][0]) for name in ("frames", "templates", "queries")}
    decoys = {name: np.ascontiguousarray(arr.reshape(-1)[::-1]).reshape(arr.shape) for name, arr in true_inputs.items()}
    decoys["queries"] = queries.copy()                                          # valid queries with the same windows ...
    decoys["queries"][:, 0] = (queries[:, 0] + 1) % len(frames)                 # ... on another frame each
    stage = {name: _hip.DeviceBuffer.from_array(arr) for name, arr in true_inputs.items()}
    blocker, stream, events = S.Blocker(be), C.c_void_p(), [C.c_void_p(), C.c_void_p()]
    try:
        be.check(L.va_stream_create(C.byref(stream)))
        for event in events:
            be.check(L.va_event_create(C.byref(event)))
        for name, arr in decoys.items():                                        # the decoys alone, on the null stream
            bufs.load(name, arr)
        assert bufs.call("ccoeff") == 0
        best, maps, clean = bufs.outputs()
        assert clean and best.tobytes() != truth[0].tobytes() and maps.tobytes() != truth[1].tobytes()
        bufs.reset()
        be.check(L.va_stream_sync(stream))
        t0 = time.perf_counter()
        be.check(L.va_event_record(events[0], stream))
        blocker.enqueue(stream)
        be.check(L.va_event_record(events[1], stream))
        for name, buf in stage.items():
            be.check(L.va_memcpy_d2d(bufs.at[name], buf.ptr, true_inputs[name].nbytes, stream))
        rc = bufs.call("ccoeff", stream=stream)
        span = time.perf_counter() - t0
        assert rc == 0
        best, maps, clean = bufs.outputs(stream)
        busy = C.c_float()
        be.check(L.va_event_elapsed_ms(events[0], events[1], C.byref(busy)))
        assert span < busy.value / 1e3, "the call returned %.2f ms after the blocker was enqueued, which held the " \
                                        "stream for %.2f ms: the call synchronised" % (span * 1e3, busy.value)
        assert clean and best.tobytes() == truth[0].tobytes() and maps.tobytes() == truth[1].tobytes()
    finally:
        L.va_stream_sync(stream)
        for event in events:
            if event.value:
                L.va_event_destroy(event)
        if stream.value:
            L.va_stream_destroy(stream)
        blocker.free()
        bufs.free()
        for buf in stage.values():
            buf.free()


# ------------------------------------------------------------------------------------------------ image and tracker
def test_image_match_template_and_find_template(cases):
    from video import ops
    from video.analysis import image
    frames, templates, _, _ = cases
    scene, t = frames[1], templates[3]
    for method in K.METHODS:
        full = image.match_template(scene, t, method=method)
        want = K.score_map(method, t, *K.sums_integral(scene, t, 0, 0, 77, 44))
        assert full.shape == (44, 77) and full.tobytes() == want.tobytes(), method
    assert image.find_template(scene, t) == ((30, 20), 1.0)
    assert image.find_template(scene, t, search_rect=(20, 10, 30, 30), method="sqdiff") == ((30, 20), 0.0)
    dev = ops.DeviceFrames.upload(frames)
    try:
        for stack in (frames, dev):
            positions, scores = image.find_template(stack, t, search_rect=(-5, 15, 60, 20), method="ccorr_normed")
            for f in range(len(frames)):
                one = K.score_map("ccorr_normed", t, *K.sums_windows(frames[f], t, 0, 15, 49, 16))
                score, i, j = K.best_of("ccorr_normed", one)
                assert (positions[f, 0], positions[f, 1]) == (i, 15 + j) and scores[f] == score, f
    finally:
        dev.release()


@pytest.fixture(scope="module")
def moving():
    """40 frames of 72 x 100: three textured patches that drift by at most 8 pixels over the clip on a noisy ground"""
    rng = np.random.default_rng(47)
    patches = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((9, 11), (12, 8), (7, 7))]
    starts, steps = ((12, 10), (60, 30), (30, 52)), ((0.2, 0.1), (-0.2, 0.15), (0.1, -0.2))
    clip = np.empty((40, 72, 100), np.uint8)
    where = np.empty((40, 3, 2), np.int32)
    for f in range(40):
        clip[f] = rng.integers(90, 110, (72, 100))
        for k, (patch, (x, y), (dx, dy)) in enumerate(zip(patches, starts, steps)):
            px, py = int(round(x + f * dx)), int(round(y + f * dy))
            clip[f, py:py + patch.shape[0], px:px + patch.shape[1]] = patch
            where[f, k] = (px, py)
    return clip, patches, starts, where


def test_template_tracker_equals_the_per_frame_loop(moving):
    from video import ops
    from video.analysis import image
    from video.analysis.tracking import TemplateTracker
    clip, patches, starts, where = moving
    radius = 10
    tracker = TemplateTracker(patches, starts, radius)
    positions, scores = tracker.update(clip)
    assert positions.dtype == np.int32 and np.array_equal(positions, where) and (scores > 0.999).all()
    assert np.array_equal(tracker.positions, where[-1])
    for k, (patch, (x, y)) in enumerate(zip(patches, starts)):
        rect = (x - radius, y - radius, 2 * radius + patch.shape[1], 2 * radius + patch.shape[0])
        for f in range(len(clip)):
            (px, py), score = image.find_template(clip[f], patch, search_rect=rect)
            assert (px, py) == tuple(positions[f, k]) and np.float64(score).tobytes() == scores[f, k].tobytes(), (f, k)
    # the batches 1 + 7 + 32 against one batch, host frames against resident ones
    dev = ops.DeviceFrames.upload(clip)
    split, at = TemplateTracker(patches, starts, radius), 0
    try:
        for count in (1, 7, 32):
            part = dev.gather(range(at, at + count))
            try:
                got_positions, got_scores = split.update(part if count != 7 else clip[at:at + count])
            finally:
                part.release()
            assert got_positions.tobytes() == positions[at:at + count].tobytes(), count
            assert got_scores.tobytes() == scores[at:at + count].tobytes(), count
            at += count
    finally:
        dev.release()
    # a patch at the frame's corner: the window is clipped, not refused
    corner = TemplateTracker([clip[0, :6, :9].copy()], [(0, 0)], radius, method="sqdiff")
    positions, scores = corner.update(clip[:1])
    assert positions.tolist() == [[[0, 0]]] and scores.tolist() == [[0.0]]
