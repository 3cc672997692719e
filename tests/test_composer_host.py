"""CPU: the composer's definitions ("Composer") and its host layer.

The restatement tests/composer_checks.py against the fixture tests/golden/composer_v1.npz (the reference's own
highlight_mask, CHANNEL_NAMES and get_color; the blend, add and drawing entries, the last redrawn from the
generator's command list, pin the restatement's bytes over time), the anchors of the
section, and VideoComposer's recording with ops.compose_layers / ops.draw replaced by the restatement through
monkeypatch (the composer looks the ops up on video.ops when a flush runs)."""
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

import composer_checks as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_composer", os.path.join(ROOT, "tests", "golden", "make_golden_composer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "composer_v1.npz"), allow_pickle=False)


@pytest.fixture
def restated_ops(monkeypatch):
    """video.ops with the two composer ops replaced by the restatement; the calls are logged"""
    from video import ops
    log = []

    def compose_layers(frames, layers, color=None, keep=False, stream=None):
        log.append(("layers", len(frames), sum(len(x) for x in layers)))
        return K.compose_layers(frames, layers, color=color)

    def draw(frames, commands, keep=False, stream=None):
        log.append(("draw", len(frames), sum(len(x) for x in commands)))
        return K.draw(frames, commands)

    def refuse(*args, **kwargs):
        raise AssertionError("this test must not reach the device")
    monkeypatch.setattr(ops, "compose_layers", compose_layers)
    monkeypatch.setattr(ops, "draw", draw)
    monkeypatch.setattr(ops, "resize", refuse)
    monkeypatch.setattr(ops, "find_contours", refuse)
    return log


# ------------------------------------------------------------------------------------------------ the fixture
def test_highlight_is_the_reference_s(fixture):
    seen = 0
    for key in fixture.files:
        if not key.startswith("ref_highlight_"):
            continue
        _, _, tag, ch, strength = key.split("_")
        ch = None if ch == "none" else (int(ch) if ch.isdigit() else ch)
        frame = fixture["ref_in_" + tag].copy()
        K.highlight(frame, fixture["ref_in_mask"], ch, int(strength))
        assert np.array_equal(frame, fixture[key]), key
        seen += 1
    assert seen == (2 + 11) * 5                     # every channel spelling, strengths 0, 1, 128, 254, 255


def test_restated_entries_still_hold(fixture):
    mono, rgb = fixture["restated_in_mono"], fixture["restated_in_rgb"]
    image, image3, mask = fixture["restated_in_image"], fixture["restated_in_image3"], fixture["restated_in_mask"]
    for w in (0.0, 1.0, 0.5, 0.3):
        assert np.array_equal(K.blend(mono.copy(), image, w, None), fixture["restated_blend_mono_%g" % w])
        assert np.array_equal(K.blend(rgb.copy(), image3, w, mask), fixture["restated_blend_rgb_%g" % w])
    assert np.array_equal(fixture["restated_blend_mono_0"], mono)
    assert np.array_equal(fixture["restated_blend_mono_1"], image)
    assert np.array_equal(K.add(mono.copy(), image, mask), fixture["restated_add_mono"])
    assert np.array_equal(K.add(rgb.copy(), image, None), fixture["restated_add_rgb"])
    G = _generator()                                # the command list is the generator's own
    assert np.array_equal(K.draw_frame(mono.copy(), G.draw_commands(1)), fixture["restated_draw_mono"])
    assert np.array_equal(K.draw_frame(rgb.copy(), G.draw_commands(3)), fixture["restated_draw_rgb"])
    assert (fixture["restated_draw_mono"] != mono).sum() > 300 and fixture["restated_draw_rgb"].shape == (48, 64, 3)


def test_channel_names_and_get_color(fixture, monkeypatch):
    from video.io import composer
    keys = [int(k) if k.isdigit() else k for k in fixture["ref_channel_keys"]]
    assert dict(zip(keys, fixture["ref_channel_values"].tolist())) == composer.CHANNEL_NAMES
    for parser in ("matplotlib", "table"):
        if parser == "table":
            monkeypatch.setattr(composer.get_color, "parser", composer._table_parser)
        for name, want in zip(fixture["ref_color_names"], fixture["ref_color_values"]):
            assert composer.get_color(str(name)) == want.tolist(), (parser, name)
        assert composer.get_color(tuple(fixture["ref_color_float_in"])) == fixture["ref_color_float_out"].tolist()
    with pytest.raises(ValueError):
        composer.get_color("no such colour")
    vc = composer.VideoComposer(None, (4, 4), 25, False)
    assert vc.get_color("g") == int(np.mean(composer.get_color("g"))) and vc.get_color("w") == 255


# ------------------------------------------------------------------------------------------------ the anchors
def test_circle_anchors():
    for r, count in enumerate((1, 5, 13, 29, 49, 81)):
        disc = set(K.circle_pixels(64, 64, 30, 30, r, True))
        ring = set(K.circle_pixels(64, 64, 30, 30, r, False))
        assert len(disc) == count and ring <= disc
        for pts in (disc, ring):                    # symmetric about both axes and the diagonal
            rel = {(x - 30, y - 30) for x, y in pts}
            assert rel == {(-x, y) for x, y in rel} == {(x, -y) for x, y in rel} == {(y, x) for x, y in rel}
    assert set(K.circle_pixels(64, 64, 5, 5, 1, True)) == {(5, 5), (4, 5), (6, 5), (5, 4), (5, 6)}
    assert K.circle_pixels(64, 64, 5, 5, -1, True) == [] and K.circle_pixels(64, 64, 5, 5, 0, False)[0] == (5, 5)
    # a disc that reaches in from outside: the full disc, intersected with the image
    full = {(x - 52, y - 47) for x, y in K.circle_pixels(100, 100, 50, 50, 4, True)}          # centred on (-2, 3)
    assert set(K.circle_pixels(8, 8, -2, 3, 4, True)) == {(x, y) for x, y in full if 0 <= x < 8 and 0 <= y < 8} != set()


def test_polyline_edge_cases():
    assert K.polyline_pixels(9, 9, np.zeros((0, 2), int), True) == []
    assert K.polyline_pixels(9, 9, np.zeros((0, 2), int), False) == []
    assert K.polyline_pixels(9, 9, [(3, 4)], False) == []
    assert K.polyline_pixels(9, 9, [(3, 4)], True) == [(3, 4)]
    assert K.polyline_pixels(9, 9, [(30, 4)], True) == []
    assert K.polyline_pixels(9, 9, [(1, 1), (4, 2)], False) == [(1, 1), (2, 1), (3, 2), (4, 2)]
    assert set(K.polyline_pixels(9, 9, [(1, 1), (4, 2)], True)) == {(1, 1), (2, 1), (3, 2), (4, 2)}
    # the line is drawn from its left end whatever the order of the points
    assert K.line_pixels(9, 9, 4, 2, 1, 1) == K.line_pixels(9, 9, 1, 1, 4, 2)
    # clipLine: the part inside, both ends moved
    pix = K.line_pixels(9, 9, -4, -2, 20, 10)
    assert pix and all(0 <= x < 9 and 0 <= y < 9 for x, y in pix) and pix[0][0] == 0
    assert K.line_pixels(9, 9, -4, 2, -1, 7) == [] and K.line_pixels(0, 0, 0, 0, 1, 1) == []
    rect = K.draw_frame(np.zeros((6, 7), np.uint8), [("polyline", [(1, 1), (5, 1), (5, 4), (1, 4)], True, 9)])
    assert rect.sum() == 9 * 14 and rect[2:4, 2:5].sum() == 0


def test_contiguous_true_regions_matches_the_restatement():
    from video.io.composer import contiguous_true_regions
    for cond in ([], [True], [False], [True, True, False, True], [False, True, True, False, False, True]):
        assert contiguous_true_regions(cond) == K.contiguous_true_regions(cond)
    assert contiguous_true_regions([False, True, True, False, True]) == [(1, 3), (4, 5)]


# ------------------------------------------------------------------------------------------------ recording
def _calls(target, t, frame, mask, image):
    target.set_frame(frame)
    target.highlight_mask(mask, "all", 100)
    target.add_image(image, mask)
    target.add_line([(3, 4), (20, 18), (-1, 2), (12, 12), (14, 19)], "r", mark_points=(t % 2 == 0))
    target.add_rectangle((2 + t, 3, 12, 9), "b")
    target.add_contour(np.array([[[4, 4]], [[15, 5]], [[9, 14]]], np.int32), "g")
    target.add_points([(6, 6), (40, 9)], 1, "y")
    target.blend_image(image, 0.25)                 # a second run of layers after the drawing
    target.add_circle((10, 10), 3, "w", thickness=1)


@pytest.mark.parametrize("is_color", (False, True))
def test_recording_flush_boundaries_and_output_period(restated_ops, is_color):
    from video.io.composer import VideoComposer, get_color
    rng = np.random.default_rng(3)
    n, h, w = 23, 20, 24
    clip = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    image = rng.integers(0, 256, (h, w), dtype=np.uint8)
    sunk = []
    vc = VideoComposer(sunk.append, (w, h), 25, is_color, output_period=2, batch=5)
    rp = K.Replay((w, h), is_color, output_period=2, get_color=get_color)
    for t in range(n):
        mask = rng.random((h, w)) < 0.4
        for target in (vc, rp):
            _calls(target, t, clip[t], mask, image)
    assert len(sunk) == 10                          # 12 output frames: two flushes of 5 so far
    vc.close()
    want = rp.close()
    assert len(sunk) == 12 and np.array_equal(np.array(sunk), want)
    # per flush: layers, draw, layers, draw -- one pair per alternation, over all pending frames
    assert [x[:2] for x in restated_ops] == [(k, m) for m in (5, 5, 2) for k in ("layers", "draw", "layers", "draw")]
    with pytest.raises(AttributeError):
        vc.frames


def test_everything_is_captured_at_call_time(restated_ops):
    from video.io.composer import VideoComposer, get_color
    h, w = 10, 12
    frame, image = np.full((h, w), 50, np.uint8), np.full((h, w), 200, np.uint8)
    mask, pts = np.zeros((h, w), bool), np.array([(1, 1), (8, 6)])
    mask[2:5, 3:9] = True
    vc = VideoComposer(None, (w, h), 25, False)
    rp = K.Replay((w, h), False, get_color=get_color)
    for target in (vc, rp):
        target.set_frame(frame)
        target.blend_image(image, 0.5, mask)
        target.add_line(pts, "w", is_closed=False)
    frame[:], image[:], mask[:], pts[:] = 0, 0, True, 3         # the caller reuses its arrays
    vc.set_frame(frame)
    vc.blend_image(image, 0.5)                                  # the same object, changed: captured anew
    got = vc.frame                                              # reading the frame flushes
    assert np.array_equal(got, np.zeros((h, w), np.uint8))
    vc.add_circle((3, 3), 0, "w")                               # the frame stays open after it was read
    vc.close()
    assert vc.frames.shape == (2, h, w) and np.array_equal(vc.frames[0], rp.close()[0])
    assert vc.frames[1].sum() == 255 and vc.frames[1][3, 3] == 255


def test_capture_is_keyed_on_the_caller_s_array(restated_ops):
    """an unchanged array is captured once, whatever its dtype; a changed one anew"""
    from video.io.composer import VideoComposer
    vc = VideoComposer(None, (6, 5), 25, False)
    for mask in (np.zeros((5, 6), bool), np.zeros((5, 6), np.uint8), np.zeros((5, 6), np.float32)):
        mask[1, 2] = 1
        first, again = vc._capture(mask, as_mask=True), vc._capture(mask, as_mask=True)
        assert again is first and first.dtype == np.uint8 and not np.shares_memory(first, mask)
        assert first[1, 2] != 0 and np.count_nonzero(first) == 1
        mask[3, 3] = 1
        changed = vc._capture(mask, as_mask=True)
        assert changed is not first and np.count_nonzero(changed) == 2 and np.count_nonzero(first) == 1
    frozen = np.arange(30, dtype=np.uint8).reshape(5, 6)
    frozen.flags.writeable = False
    assert vc._capture(frozen) is vc._capture(frozen)


def test_value_errors_and_unsupported_calls(restated_ops):
    from video.io.composer import VideoComposer
    h, w = 8, 9
    mono, rgb = VideoComposer(None, (w, h), 25, False), VideoComposer(None, (w, h), 25, True)
    frame, frame3 = np.zeros((h, w), np.uint8), np.zeros((h, w, 3), np.uint8)
    mask = np.ones((h, w), bool)
    with pytest.raises(ValueError):
        mono.set_frame(frame3)                      # a colour frame in a monochrome video
    with pytest.raises(ValueError):
        mono.set_frame(frame[:4])
    with pytest.raises(ValueError):
        VideoComposer(None, (w, h), 25, False, batch=0)
    mono.set_frame(frame)
    rgb.set_frame(frame)
    for call in (lambda: mono.highlight_mask(mask, "r"), lambda: rgb.highlight_mask(mask, "x"),
                 lambda: rgb.highlight_mask(mask, "all", 256), lambda: rgb.highlight_mask(mask, "all", -1),
                 lambda: rgb.highlight_mask(mask, "all", 12.5), lambda: rgb.highlight_mask(mask[:3]),
                 lambda: mono.add_image(frame3), lambda: mono.blend_image(frame3), lambda: rgb.add_image(frame[:5]),
                 lambda: rgb.blend_image(frame, 0.5, mask[:, :2]), lambda: rgb.blend_image(frame, float("nan")),
                 lambda: rgb.add_line([(1, 1), (1 << 21, 5)]), lambda: rgb.add_rectangle((0, 0, 1 << 21, 4))):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: rgb.add_contour([np.zeros((3, 1, 2), np.int32)], thickness=2),
                 lambda: rgb.add_contour([np.zeros((3, 1, 2), np.int32)], thickness=-1),
                 lambda: rgb.add_line([(1, 1), (2, 2)], width=3), lambda: rgb.add_rectangle((0, 0, 3, 3), width=2),
                 lambda: rgb.add_circle((1, 1), 2, thickness=2), lambda: rgb.add_text("worm", (2, 2))):
        with pytest.raises(NotImplementedError):
            call()
    rgb.add_circle((float("nan"), 2), 2)            # the reference swallows what int() refuses
    rgb.add_circle((1 << 40, 2), 2)
    assert rgb._pending[-1].steps == [] and mono._pending[-1].steps == []


def test_skipped_frames_record_nothing(restated_ops):
    from video.io.composer import VideoComposer
    vc = VideoComposer(None, (6, 5), 25, False, output_period=3)
    frame = np.zeros((5, 6), np.uint8)
    for t in range(7):
        vc.set_frame(frame + t)
        vc.add_circle((2, 2), 0, "w")
        if t % 3:
            vc.highlight_mask("not even an array", "nonsense", 999)      # skipped before anything is looked at
            assert not vc.output_this_frame
    assert len(vc._pending) == 3 and all(len(p.steps) == 1 for p in vc._pending)
    vc.close()
    assert vc.frames[:, 0, 0].tolist() == [0, 3, 6] and (vc.frames[:, 2, 2] == 255).all()


def test_zoom_coordinates_are_the_reference_s_expressions(restated_ops, monkeypatch):
    from video import ops
    from video.io.composer import VideoComposer
    zoom = 3
    monkeypatch.setattr(ops, "resize", lambda frames, size, interpolation="linear", color=False:
                        np.zeros((len(frames), size[1], size[0]) + ((3,) if color else ()), np.uint8))
    vc = VideoComposer(None, (60, 45), 25, False, zoom_factor=zoom)
    assert vc.size == (20, 15)
    vc.set_frame(np.zeros((45, 60), np.uint8))
    pts = np.array([(10, 11), (29.9, 44.0), (31, 2)])
    vc.add_line(pts, "w")
    vc.add_circle((29.9, 44), 5, "w")
    vc.add_rectangle((10, 11, 20, 8), "w", width=3)              # ceil(3 / 3) = 1: still thickness 1
    vc.add_contour(np.array([[[7, 8]], [[50, 40]]], np.int32), thickness=2)
    steps = [item for _, item in vc._pending[-1].steps]
    assert np.array_equal(steps[0][1], (pts / zoom).astype(int)) and steps[0][1].tolist()[1] == [9, 14]
    assert steps[1][1:4] == ((int(29.9 / zoom), int(44 / zoom)), int(np.ceil(5 / zoom)), True)
    rect = np.asarray((10, 11, 20, 8)) / zoom
    x1, y1, x2, y2 = int(rect[0]), int(rect[1]), int(rect[0] + rect[2] - 1), int(rect[1] + rect[3] - 1)
    assert steps[2][1].tolist() == [[x1, y1], [x2, y1], [x2, y2], [x1, y2]]
    assert steps[3][1].tolist() == [[2, 2], [16, 13]]
    with pytest.raises(NotImplementedError):
        vc.add_line(pts, "w", width=4)
    vc.close()
    assert vc.frames.shape == (1, 15, 20)


def test_product_does_not_import_the_restatement():
    pkg = os.path.join(ROOT, "video-analysis_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                assert "composer_checks" not in open(os.path.join(dirpath, f)).read(), f


# ------------------------------------------------------------------------------------------------ the header
def test_raster_header_on_the_host_under_sanitizers(tmp_path):
    """va_raster.h compiled for the host with -fsanitize=address,undefined into a stand-alone program that
    rasterises clip cases and circles; its pixels are the restatement's"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")         # the Makefile's compiler: its clang++ builds host code too
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "llvm", "bin", "clang++")
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or (
        rocm_clang if os.path.exists(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler: neither g++, c++ or clang++ on the PATH nor %s" % rocm_clang
    exe = str(tmp_path / "raster_shim")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "video-analysis_amd", "csrc"),
                           os.path.join(ROOT, "tests", "raster_shim.cpp"), "-o", exe])
    w, h = 53, 37
    segs = [(-10, 5, 20, 30), (20, 30, 80, 8), (-7, -3, 70, 50), (-20, 10, -3, 30), (5, -40, 60, -2), (60, 20, 10, 90),
            (-5, 36, 58, 37), (52, -9, 53, 44), (-1000000, -999999, 1000000, 1048576), (7, 7, 7, 7), (40, 3, 2, 30)]
    circles = [(20, 15, r, f) for r in (0, 1, 2, 5, 20) for f in (0, 1)] + [(-4, 18, 6, 1), (60, -3, 20, 0), (3, 3, -1, 1)]
    text = "%d %d\n" % (w, h) + "".join("L %d %d %d %d\n" % s for s in segs) + "".join("C %d %d %d %d\n" % c for c in circles)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    got = [sorted(tuple(int(v) for v in p.split(",")) for p in line.split()) for line in out[:len(segs) + len(circles)]]
    want = [sorted(K.line_pixels(w, h, *s)) for s in segs] + [sorted(K.circle_pixels(w, h, x, y, r, bool(f)))
                                                               for x, y, r, f in circles]
    assert got == want
