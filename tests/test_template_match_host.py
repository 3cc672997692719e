"""CPU: template matching of DESIGN.md §9, "Template matching".  The two restatements agree with the fixture; the entry
points are declared, exported and bound; the ctypes structs have the header's sizes and offsets; the entry point
refuses bad arguments before a device is touched; the workspace formula; va_template_match_math.h, compiled with the
host compiler under sanitizers into a stand-alone program, gives the fixture's bests and maps for every method; the
argument checks of ops.match_templates, image.match_template / find_template and TemplateTracker, and their clipping
and plumbing on a NumPy model of the call.  Comparisons are exact."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import template_match_checks as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "videoanalysis_hip.h")
INVALID = -22


@pytest.fixture(scope="module")
def cases():
    return K.fixture()


def test_fixture_covers_the_shapes_windows_and_statuses(cases):
    frames, templates, queries, want = cases
    assert frames.dtype == np.uint8 and frames.shape[2] % 4 != 0
    shapes = {t.shape for t in templates}
    assert shapes >= {(1, 1), (1, 5), (3, 4), (5, 7), (16, 16), (33, 17), (K.CHUNK_ROWS + 1, 6), (2, K.CHUNK_COLS + 6)}
    status = want["sqdiff"][0]["status"]
    assert set(status.tolist()) >= {0, K.BAD_FRAME, K.BAD_TEMPLATE, K.EMPTY, K.OUTSIDE, K.BAD_FRAME | K.BAD_TEMPLATE | K.EMPTY}
    good = queries[status == 0]
    for size in (1, K.TILE - 1, K.TILE, K.TILE + 1, 2 * K.TILE + 1):
        assert size in good[:, 4] and (size in good[:, 5] or size > 40), size
    h, w = frames.shape[1:]
    th, tw = np.array([templates[t].shape for t in good[:, 1]]).T
    assert (good[:, 2] == 0).any() and (good[:, 3] == 0).any()                  # windows at all four edges
    assert (good[:, 2] + good[:, 4] - 1 + tw == w).any() and (good[:, 3] + good[:, 5] - 1 + th == h).any()
    # zero denominators and ties are in it: a flat template on a flat window, a zero frame, a constant frame
    best, maps = want["ccoeff_normed"]
    flat = [k for k, q in enumerate(queries) if status[k] == 0 and q[0] == 2]
    assert flat and all((maps[k] == 0.0).all() and (best["x"][k], best["y"][k]) == tuple(queries[k, 2:4]) for k in flat)
    zero = [k for k, q in enumerate(queries) if status[k] == 0 and q[0] == 3]
    assert zero and all((want["sqdiff_normed"][1][k] == 1.0).all() for k in zero)
    assert best["score"].max() == 1.0                                           # a planted template is found exactly


def test_restatements_agree_with_the_fixture(cases):
    frames, templates, queries, want = cases
    for method in K.METHODS:
        K.same_results(K.restate(frames, templates, queries, method, K.sums_windows), want[method], method)
        K.same_results(K.restate(frames, templates, queries, method, K.sums_integral), want[method], method)
    # the sums of the 256 x 256 template of 255s: beyond 2^31, below 2^32
    assert 2 ** 31 < 255 * 255 * K.MAX_PIXELS < 2 ** 32


def test_entry_points_are_declared_exported_and_bound():
    from video import _hip
    text = open(HEADER).read()
    pinned = {
        "va_template_match_workspace_bytes": ("size_t", ["int64_t", "int64_t", "int64_t"],
                                              (C.c_size_t, [C.c_int64] * 3)),
        "va_template_match_u8": ("int", ["const va_match_args *"], (C.c_int, [C.POINTER(_hip.va_match_args)])),
    }
    lib = _hip.load_library()
    for name, (result, args, bound) in pinned.items():
        found = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert found and found.group(1) == result, name + " is not declared"
        types = [re.sub(r"\s*\w+$", "", " ".join(arg.split())) for arg in found.group(2).split(",")]
        assert types == args, name
        assert hasattr(lib, name) and _hip.SIGNATURES[name] == bound, name
    for name, value in _hip.MATCH_METHODS.items():
        assert re.search(r"#define VA_MATCH_%s %d\b" % (name.upper(), value), text), name
        assert K.METHODS[value] == name
    assert re.search(r"#define VA_MATCH_TILE %d\b" % K.TILE, text)
    assert re.search(r"#define VA_MATCH_CHUNK_ROWS %d\b" % K.CHUNK_ROWS, text)
    assert re.search(r"#define VA_MATCH_CHUNK_COLS %d\b" % K.CHUNK_COLS, text)


def test_ctypes_structs_have_the_headers_sizes_and_offsets(tmp_path):
    from video import _hip
    structs = {"va_match_query": _hip.va_match_query, "va_match_best": _hip.va_match_best,
               "va_match_args": _hip.va_match_args}
    lines = []
    for name, struct in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        for field, _ in struct._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, field, name, field))
    source = tmp_path / "layout.c"
    source.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "videoanalysis_hip.h"\nint main(void)\n{\n%s\nreturn 0;\n}\n'
                      % "\n".join(lines))
    cc = K.host_compiler()
    exe = str(tmp_path / "layout")
    subprocess.check_call([cc, "-x", "c", "-I", os.path.join(ROOT, "include"), str(source), "-o", exe])
    said = dict(line.split() for line in subprocess.check_output([exe]).decode().splitlines())
    for name, struct in structs.items():
        assert int(said[name]) == C.sizeof(struct), name
        for field, _ in struct._fields_:
            assert int(said["%s.%s" % (name, field)]) == getattr(struct, field).offset, (name, field)
    assert C.sizeof(_hip.va_match_query) == 24 and C.sizeof(_hip.va_match_best) == 24
    assert C.sizeof(_hip.va_match_args) == 144
    assert _hip.MATCH_QUERY_DTYPE.itemsize == 24 and _hip.MATCH_BEST_DTYPE.itemsize == 24 and K.BEST_DTYPE == _hip.MATCH_BEST_DTYPE


def good_args(**changes):
    """arguments that pass every check (made-up addresses, never dereferenced), with `changes` applied"""
    from video import _hip
    lib = _hip.load_library()
    P = 1 << 20
    fields = dict(struct_size=C.sizeof(_hip.va_match_args), method=5, frames_dev=P, n=2, h=40, w=50, reserved=0,
                  frame_stride=2000, templates_dev=2 * P, template_shapes_dev=3 * P, template_offsets_dev=4 * P,
                  n_templates=3, queries_dev=5 * P, n_queries=7, total_positions=900, best_out_dev=6 * P,
                  maps_out_dev=7 * P, map_offsets_dev=8 * P, workspace_dev=9 * P,
                  workspace_bytes=lib.va_template_match_workspace_bytes(7, 900, 3), stream=None)
    fields.update(changes)
    return _hip.va_match_args(**fields)


def test_entry_point_refuses_bad_arguments_before_a_device():
    from video import _hip
    lib = _hip.load_library()
    P = 1 << 20

    def refused(words, **changes):
        rc = lib.va_template_match_u8(C.byref(good_args(**changes)))
        said = lib.va_last_error().decode()
        return rc == INVALID and said.startswith("va_template_match_u8: ") and words in said, (rc, said)

    assert lib.va_template_match_u8(None) == INVALID
    for words, changes in (("struct_size", dict(struct_size=140)), ("struct_size", dict(struct_size=0)),
                           ("unknown method", dict(method=6)), ("unknown method", dict(method=-1)),
                           ("2^29 pixels", dict(h=1 << 15, w=1 << 14)), ("bad shape", dict(h=0)),
                           ("bad shape", dict(n=-1)), ("frame stride", dict(frame_stride=1999)),
                           ("counts are", dict(n_queries=-1)), ("counts are", dict(total_positions=-1)),
                           ("counts are", dict(n_templates=-1)), ("counts are", dict(total_positions=1 << 37)),
                           ("NULL argument", dict(queries_dev=None)), ("NULL argument", dict(frames_dev=None)),
                           ("NULL argument", dict(workspace_dev=None)), ("NULL argument", dict(templates_dev=None)),
                           ("NULL argument", dict(map_offsets_dev=None)),
                           ("aligned", dict(queries_dev=5 * P + 2)), ("aligned", dict(template_shapes_dev=3 * P + 1)),
                           ("aligned", dict(template_offsets_dev=4 * P + 4)), ("aligned", dict(best_out_dev=6 * P + 4)),
                           ("aligned", dict(maps_out_dev=7 * P + 4)), ("aligned", dict(map_offsets_dev=8 * P + 4)),
                           ("aligned", dict(workspace_dev=9 * P + 4)),
                           ("workspace of", dict(workspace_bytes=lib.va_template_match_workspace_bytes(7, 900, 3) - 1)),
                           ("workspace of", dict(total_positions=100000))):
        ok, seen = refused(words, **changes)
        assert ok, (words, changes, seen)
    # no queries: nothing to do, whatever the pointers, and no device
    assert lib.va_template_match_u8(C.byref(good_args(n_queries=0, queries_dev=None, workspace_dev=None))) == 0


def test_workspace_formula():
    from video import _hip
    lib = _hip.load_library()

    def up(v):
        return (v + 255) // 256 * 256
    for nq, positions, m in ((0, 0, 0), (1, 1, 1), (7, 900, 3), (70000, 70000, 1), (10240, 10240 * 65 * 65, 40)):
        tiles = nq + positions // K.TILE + positions // (K.TILE * K.TILE) + 1
        assert lib.va_template_match_workspace_bytes(nq, positions, m) == up(8 * m) + up(8 * (nq + 2)) + up(24 * tiles)
    # the bound holds for every window shape
    for nx in range(1, 3 * K.TILE + 2):
        for ny in (1, 2, K.TILE - 1, K.TILE, K.TILE + 1, 100):
            tiles = -(-nx // K.TILE) * -(-ny // K.TILE)
            assert tiles <= 1 + nx * ny // K.TILE + nx * ny // (K.TILE * K.TILE) + 1
    for bad in ((-1, 0, 0), (0, -1, 0), (0, 0, -1), (1 << 31, 0, 0), (1, 1 << 37, 1)):
        assert lib.va_template_match_workspace_bytes(*bad) == 0


def test_math_header_on_the_host_under_sanitizers(cases, tmp_path):
    frames, templates, queries, want = cases
    exe = K.compile_shim(tmp_path)
    px = frames.shape[1] * frames.shape[2]
    runs = [(frames, px + (0, 5, 4)[i % 3], templates, queries, method) for i, method in enumerate(K.METHODS)]
    # ties across tiles: a constant frame, and two planted equal bests in different tiles
    planted = np.full((1, 40, 80), 9, np.uint8)
    planted[0, 3:5, 70:73] = planted[0, 36:38, 2:5] = np.array([[200, 0, 200], [0, 200, 0]], np.uint8)
    tie_templates = [planted[0, 3:5, 70:73].copy()]
    tie_queries = np.array([(0, 0, 0, 0, 78, 39)], np.int32)
    runs += [(planted, 3200, tie_templates, tie_queries, method) for method in K.METHODS]
    got = K.run_shim(exe, runs)
    for i, method in enumerate(K.METHODS):
        K.same_results(got[i], want[method], method)
        ties = K.restate(planted, tie_templates, tie_queries, method)
        K.same_results(got[len(K.METHODS) + i], ties, method)
        if method != "ccorr":
            assert (ties[0]["x"][0], ties[0]["y"][0]) == (70, 3), method         # the earlier of the two in raster order


class NumpyMatcher(object):
    """ops.match_templates on the window restatement, for the plumbing tests; it records its calls"""

    def __init__(self):
        self.calls = []

    def __call__(self, frames, templates, queries, method="ccoeff_normed", maps=False, keep=False, stream=None):
        from video import ops
        frames, queries = np.asarray(frames), np.asarray(queries, np.int32).reshape(-1, 6)
        self.calls.append((frames.shape, len(templates), queries.copy(), method))
        best, score_maps = K.restate(frames, templates, queries, method)
        out = np.zeros(len(best), ops.MATCH_RESULT_DTYPE)
        for name in ("score", "x", "y", "status"):
            out[name] = best[name]
        return (out, score_maps) if maps else out


def test_host_status_model_equals_the_restated_rule(cases):
    from video import ops
    frames, templates, queries, want = cases
    shapes = [t.shape for t in templates]
    status = ops.match_query_status(ops.match_query_table(queries), len(frames), frames.shape[1], frames.shape[2], shapes)
    assert np.array_equal(status, want["ccorr"][0]["status"])
    records = np.zeros(len(queries), ops._hip.MATCH_QUERY_DTYPE)
    for k, name in enumerate(records.dtype.names):
        records[name] = queries[:, k]
    assert np.array_equal(ops.match_query_table(records), queries)
    assert np.array_equal(ops.match_query_status(ops.match_query_table(queries), 0, 48, 83, shapes) & K.BAD_FRAME,
                          np.full(len(queries), K.BAD_FRAME))


def test_argument_checks_raise_before_a_device_is_touched(monkeypatch):
    from video import _hip, ops
    from video.analysis import image
    from video.analysis.tracking import TemplateTracker

    def no_device(*a, **k):
        raise AssertionError("an argument check came after the device was asked for")
    monkeypatch.setattr(_hip, "lib", no_device)
    u8, t = np.zeros((3, 20, 30), np.uint8), np.zeros((4, 5), np.uint8)
    query = [(0, 0, 0, 0, 2, 2)]
    for bad in (u8.astype(np.int16), u8.astype(np.float32), u8.astype(bool)):
        with pytest.raises(TypeError):
            ops.match_templates(bad, [t], query)
        with pytest.raises(TypeError):
            ops.match_templates(u8, [bad[0]], query)
        with pytest.raises(TypeError):
            image.match_template(bad[0], t)
        with pytest.raises(TypeError):
            image.find_template(u8, bad[0])
    for bad_shape in (u8[0], np.zeros((3, 20, 30, 3), np.uint8), np.zeros((3, 20, 30, 2), np.uint8)):
        with pytest.raises(ValueError):
            ops.match_templates(bad_shape, [t], query)
    for bad_template in (np.zeros((0, 4), np.uint8), np.zeros(7, np.uint8), np.zeros((257, 256), np.uint8),
                         np.zeros((2, 3, 4), np.uint8)):
        with pytest.raises(ValueError):
            ops.match_templates(u8, [t, bad_template], query)
    for bad_queries in ([(0, 0, 0, 0, 2)], np.zeros((2, 6)), [(0, 0, 0, 0, 2, 1 << 31)], np.zeros((2, 3, 6), np.int32)):
        with pytest.raises(ValueError):
            ops.match_templates(u8, [t], bad_queries)
    for bad_method in ("TM_CCOEFF", 5, None, "ccoeff-normed"):
        with pytest.raises(ValueError):
            ops.match_templates(u8, [t], query, method=bad_method)
        with pytest.raises(ValueError):
            TemplateTracker([t], [(1, 1)], 3, method=bad_method)
    with pytest.raises(ValueError):
        image.match_template(u8[0], np.zeros((21, 5), np.uint8))                # the template does not fit
    with pytest.raises(ValueError):
        image.find_template(u8, t, search_rect=(0, 0, 4, 4))                    # ... nor in the rectangle
    with pytest.raises(ValueError):
        image.find_template(u8, t, search_rect=(27, 0, 10, 10))                 # ... nor in what the frame leaves of it
    with pytest.raises(RuntimeError):
        image.find_template(u8, t, search_rect=(30, 0, 10, 10))                 # get_overlapping_slices: no overlap
    for bad_radius in (-1, 2.5, None, True):
        with pytest.raises(ValueError):
            TemplateTracker([t], [(1, 1)], bad_radius)
    with pytest.raises(ValueError):
        TemplateTracker([t, t], [(1, 1)], 3)
    with pytest.raises(ValueError):
        TemplateTracker([], [], 3)
    with pytest.raises(TypeError):
        TemplateTracker([t], [(1, 1)], 3).update(u8.astype(np.float32))
    # nothing to do needs no device either
    empty = ops.match_templates(u8, [t], np.zeros((0, 6), np.int32))
    assert empty.shape == (0,) and empty.dtype == ops.MATCH_RESULT_DTYPE
    none, maps = ops.match_templates(u8[:0], [t], query, maps=True)
    assert none["status"].tolist() == [K.BAD_FRAME] and np.isnan(none["score"][0]) and maps[0].shape == (0, 0)
    positions, scores = TemplateTracker([t], [(1, 1)], 3).update(u8[:0])
    assert positions.shape == (0, 1, 2) and scores.shape == (0, 1)


def test_search_windows_are_clipped_as_get_overlapping_slices_clips():
    from video.analysis import image, regions
    shape = (40, 60)                                                            # (height, width)
    assert image.template_search_window(None, (5, 7), shape) == (0, 0, 54, 36)
    assert image.template_search_window((10, 8, 20, 12), (5, 7), shape) == (10, 8, 14, 8)
    assert image.template_search_window((-4, -3, 20, 12), (5, 7), shape) == (0, 0, 10, 5)
    assert image.template_search_window((50, 33, 20, 12), (5, 7), shape) == (50, 33, 4, 3)
    assert image.template_search_window((53, 35, 7, 5), (5, 7), shape) == (53, 35, 1, 1)
    for rect in ((10, 8, 20, 12), (-4, -3, 20, 12), (50, 33, 20, 12)):
        _, common = regions.get_overlapping_slices(rect[:2], (rect[3], rect[2]), shape, anchor="upper left", ret_rect=True)
        x0, y0, nx, ny = image.template_search_window(rect, (5, 7), shape)
        assert (x0, y0, nx + 7 - 1, ny + 5 - 1) == common


def test_image_and_tracker_plumbing_on_a_numpy_model(monkeypatch, cases):
    from video import ops
    from video.analysis import image
    from video.analysis.tracking import TemplateTracker
    frames, templates, _, _ = cases
    model = NumpyMatcher()
    monkeypatch.setattr(ops, "match_templates", model)
    scene, t = frames[1], templates[3]                                          # 5 x 7, planted at (30, 20)
    for method in K.METHODS:
        full = image.match_template(scene, t, method=method)
        want = K.score_map(method, t, *K.sums_windows(scene, t, 0, 0, 77, 44))
        assert full.tobytes() == want.tobytes() and full.shape == (44, 77)
    assert image.find_template(scene, t) == ((30, 20), 1.0)
    assert image.find_template(scene, t, search_rect=(20, 10, 30, 30), method="sqdiff") == ((30, 20), 0.0)
    assert model.calls[-1][2].tolist() == [[0, 0, 20, 10, 24, 26]]
    positions, scores = image.find_template(frames, t, search_rect=(-5, 15, 60, 20))
    assert positions.shape == (5, 2) and positions.dtype == np.int32 and scores.shape == (5,)
    assert model.calls[-1][2].tolist() == [[f, 0, 0, 15, 49, 16] for f in range(5)]
    assert tuple(positions[1]) == (30, 20) and scores[1] == 1.0
    # the tracker: windows of the radius around the start positions, clipped; the last frame centres the next batch
    clip = np.stack([np.roll(scene, (dy, dx), axis=(0, 1)) for dx, dy in ((0, 0), (1, 0), (2, 1), (3, 1))])
    tracker = TemplateTracker([t, templates[0]], [(29, 19), (0, 47)], 4)
    assert tracker.queries(2, scene.shape).tolist() == [[0, 0, 25, 15, 9, 9], [0, 1, 0, 43, 5, 5],
                                                        [1, 0, 25, 15, 9, 9], [1, 1, 0, 43, 5, 5]]
    positions, scores = tracker.update(clip[:3])
    assert positions.shape == (3, 2, 2) and scores.shape == (3, 2)
    assert positions[:, 0].tolist() == [[30, 20], [31, 20], [32, 21]] and (scores[:, 0] == 1.0).all()
    assert tracker.positions[0].tolist() == [32, 21]
    positions, _ = tracker.update(clip[3:])
    assert model.calls[-1][2][0].tolist() == [0, 0, 28, 17, 9, 9] and positions[0, 0].tolist() == [33, 21]


def test_good_arguments_fail_loudly_without_a_gpu():
    from video import _hip, ops
    from video.analysis import image
    from video.analysis.tracking import TemplateTracker
    u8, t = np.zeros((3, 20, 30), np.uint8), np.zeros((4, 5), np.uint8)
    if not _hip.gpu_available():
        with pytest.raises(_hip.HipUnavailableError):
            ops.match_templates(u8, [t], [(0, 0, 0, 0, 2, 2)])
        with pytest.raises(_hip.HipUnavailableError):
            image.match_template(u8[0], t)
        with pytest.raises(_hip.HipUnavailableError):
            image.find_template(u8, t)
        with pytest.raises(_hip.HipUnavailableError):
            TemplateTracker([t], [(1, 1)], 3).update(u8)
