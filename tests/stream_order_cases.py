"""Every stream-taking entry point in stream order on a busy stream: the declarations, the extra cases and the runner
("Stream order").

The header promises that every call is enqueued on its `stream` and that nothing synchronises unless stated; the
scratch lease adds that a call touches a leased block in stream order only.  On the null stream, or on an idle created
stream, a launch, fill or copy on the wrong stream still finds its inputs ready, so the other suites cannot see a breach.
Here every case of tests/pointer_offset_cases.py, and the cases below for the entry points that table lacks, runs on
one va_stream_create stream three times:

  plain        inputs uploaded and synchronised, the call on the stream, synchronise, compare bit for bit;
  gated        the working inputs hold a decoy (a second valid payload) and the outputs a sentinel; behind a blocker
               on the stream the true payloads are copied in (va_memcpy_d2d), the entry point is called, the outputs
               are copied to keep buffers and the decoys copied back, all on the stream, then one synchronisation.
               Work that is not in stream order meets the decoy or the sentinel;
  gated + fill the same under va_test_hook_fill(0): the lease zeroes its block on the stream, behind the blocker, so
               whatever the host wrote into the block ahead of the stream is gone before a kernel reads it.

Between the plain and the gated run another case of another size runs on the same stream, unsynchronised, so that
the lease hands a block from one geometry to the other.  A call is *covered* when it returned within the time the
blocker alone kept the stream busy (measured with events): every entry point declared `asynchronous` must be.
"""
import ctypes as C
import os
import re
import time

import numpy as np

import pointer_offset_cases as P
from pointer_offset_cases import Arg, Case, out

ROOT = P.ROOT
HEADER = os.path.join(ROOT, "include", "videoanalysis_hip.h")
SENTINEL = 0xA5

# ------------------------------------------------------------------------------------------- declarations
# The entry points that wait for their stream inside the call, and what for (the hipStreamSynchronize and blocking
# hipMemcpy sites of csrc/).  Every other prototype with a `void *stream` is asynchronous: it returns while the
# stream is still busy with earlier work.
SYNCHRONISES = {
    "va_memcpy_h2d": "pageable host memory: waits for the stream, then copies with a blocking copy (va_api.hip)",
    "va_memcpy_d2h": "pageable host memory: waits for the stream, then copies with a blocking copy (va_api.hip)",
    "va_stream_sync": "its purpose",
    "va_stream_destroy": "waits for the stream before its cached scratch is freed (va_api.hip)",
    "va_resize_u8": "waits for the stream before the blocking upload of its tables into leased scratch (va_resize.hip)",
    "va_resize_f32": "waits for the stream before the blocking upload of its tables into leased scratch (va_resize.hip)",
    "va_optical_flow_farneback": "waits for the stream before its pyramid's resize tables are uploaded (va_optflow.hip)",
    "va_guo_hall_thinning_u8": "reads the changed flags back every poll_period launches (va_thinning.hip)",
    "va_mask_thinning_u8": "reads the survivor counters back once per 16 iterations (va_stencil.hip)",
}

# Prototypes with a stream that have no case, and why.
EXCLUDED = {
    "va_memcpy_h2d": "the runner's instrument; pageable copies have a direct test (test_gpu_stream_order.py)",
    "va_memcpy_d2h": "the runner's instrument; pageable copies have a direct test (test_gpu_stream_order.py)",
    "va_memcpy_d2d": "the runner's instrument",
    "va_memset": "the runner's instrument",
    "va_stream_sync": "the runner's instrument",
    "va_stream_destroy": "the runner's instrument",
    "va_event_record": "the runner's instrument",
    "va_stream_wait_event": "an instrument between two streams: it has a direct test (test_gpu_stream_order.py)",
    "va_gather_counts": "needs a communicator",
}
# Synchronising cases that have nothing to wait for: an area shrink by integer factors, which the exact 2 x 2 linear
# shrink is too, uploads no table (va_resize.hip, area_fast).  Every other synchronising case must return behind the
# blocker: the header's sentence is held in both directions.
NOTHING_TO_WAIT_FOR = ("resize_u8[24x40->12x20,linear]", "resize_u8[24x40->12x20,area]")
# Outputs that depend on no input with a decoy, so that the decoy cannot change them: the split decoder's rounds are a
# property of the entropy-coded bytes, which have no decoy (reversed, they are no JPEG stream).
DECOY_BLIND = {"jpeg_decode_split_u8[2x48x64,4:2:0]": ("rounds",)}


def header_prototypes():
    """[(name, the comment in front of it or of the prototypes it follows, takes a stream)] of the header"""
    with open(HEADER) as f:
        text = f.read()
    tokens = re.findall(r"/\*.*?\*/|(?:int|size_t|const char \*|void)\s+\*?va_\w+\([^;{]*\);", text, re.S)
    found, comment = [], ""
    for tok in tokens:
        if tok.startswith("/*"):
            comment = tok
        else:
            found.append((re.search(r"(va_\w+)\(", tok).group(1), comment, bool(re.search(r"void \*stream\b", tok))))
    return found


def stream_prototypes():
    return [name for name, _, takes in header_prototypes() if takes]


def header_says_synchronises(comment):
    """the wording the header keeps for it: "synchronises `stream`" (line breaks of the comment aside)"""
    return bool(re.search(r"synchronises `stream`", re.sub(r"\s*\n\s*\*\s*", " ", comment), re.I))


def declared_class(entry):
    """"synchronises" or "asynchronous", for any prototype that takes a stream"""
    return "synchronises" if entry in SYNCHRONISES else "asynchronous"


def synchronises(case):
    return any(declared_class(e) == "synchronises" for e in case.entries)


# ------------------------------------------------------------------------------------------------ cases
# Cases for the stream suite only: the entry points that choose no kernel by a pointer's address.  Inputs and
# references are the families' own, at their smallest shapes.
EXTRA = []


def _add(*a, **kw):
    case = Case(*a, **kw)
    assert case.name not in P.BY_NAME and case.name not in {c.name for c in EXTRA}, case.name
    EXTRA.append(case)
    return case


NONE = "none (stream suite only)"


def _noise_cases():
    # va_gaussian_noise has no inputs; its reference is its own seeded output on the null stream, as the hostile-
    # memory suite pins it (self_reference: the runner computes it with the case's own call)
    for dt, code in ((np.uint8, P.VA_U8), (np.float32, P.VA_F32), (np.float64, P.VA_F64)):
        count = 4096 + 19
        case = _add("gaussian_noise[%s]" % np.dtype(dt).name, "va_gaussian_noise", NONE, [out("dst", (count,), dt)],
                    lambda L, p, _, code=code, count=count: L.va_gaussian_noise(p["dst"], code, count, 100.0, 30.0, 12345, 77,
                                                                                P.ON.stream),
                    None)
        case.self_reference = True


_noise_cases()


def _sliding_median_cases():
    import sliding_median_checks as K
    for window, px in ((3, 129), (300, 17)):               # uint8 and uint16 counters; a tile and a pixel, a part tile
        n = K.frames_of(window) if window < 10 else 12
        frames = K.content("noise", n, px, np.random.default_rng(window + px))
        zero = np.zeros(K.state_bytes(px, window), np.uint8)
        lower, upper, diff, cur_lower, cur_upper = K.restate_histogram(frames, window, ret_current=True)
        _add("sliding_median_u8[w%d,px%d]" % (window, px), ("va_sliding_median_u8", "va_sliding_median_state_bytes"), NONE,
             [Arg("frames", "in", frames), Arg("state", "work", zero, offsets=(0,)), out("lower", (n, px), np.uint8),
              out("upper", (n, px), np.uint8), out("diff", (n, px), np.uint8)],
             lambda L, p, _, n=n, px=px, window=window: L.va_sliding_median_u8(
                 p["frames"], n, px, px, window, 0, p["state"], p["lower"], p["upper"], p["diff"], P.ON.stream),
             lambda O, r=(lower, upper, diff): dict(zip(("lower", "upper", "diff"), r)))
        _add("sliding_median_current[w%d,px%d]" % (window, px), ("va_sliding_median_u8", "va_sliding_median_current"), NONE,
             [Arg("frames", "in", frames), Arg("state", "work", zero, offsets=(0,)), out("lower", (px,), np.uint8),
              out("upper", (px,), np.uint8)],
             lambda L, p, _, n=n, px=px, window=window: P._first(
                 L.va_sliding_median_u8(p["frames"], n, px, px, window, 0, p["state"], None, None, None, P.ON.stream),
                 L.va_sliding_median_current(p["state"], px, window, n, p["lower"], p["upper"], P.ON.stream)),
             lambda O, r=(cur_lower, cur_upper): dict(zip(("lower", "upper"), r)))


_sliding_median_cases()


def _contour_moment_cases():
    masks = P.blob_masks(2, 17, 70, seed=71)

    def contours(O):
        """the longest first (a single pixel's moments are all zero)"""
        found = [np.asarray(c, np.int32).reshape(-1, 2) for m in masks for c in O.find_contours_external_simple(m)]
        return sorted(found, key=len, reverse=True)

    def moments(O, curves):
        return np.array([[O.contour_moments(c)[k] for k in O.MOMENT_KEYS[:10]] for c in curves], np.float64)
    m, cap = 4, 256                                           # (asserted below: the masks have that many contours)

    def table(O):
        flat = contours(O)[:m]
        assert len(flat) == m and max(len(c) for c in flat) <= cap
        t = np.zeros((m, cap, 2), np.int32)
        for k, c in enumerate(flat):
            t[k, :len(c)] = c
        return t
    _add("contour_moments[4 contours]", "va_contour_moments", NONE,
         [Arg("points", "in", table, nbytes=m * cap * 8, itemsize=4),
          Arg("npoints", "scratch", lambda O: np.array([len(c) for c in contours(O)[:m]], np.int32), nbytes=m * 4, itemsize=4),
          out("moments", (m, 10), np.float64)],
         lambda L, p, _: L.va_contour_moments(p["points"], p["npoints"], m, cap, 0, p["moments"], P.ON.stream),
         lambda O: {"moments": moments(O, contours(O)[:m])})

    def ragged(O):
        return [c.astype(np.float32) + np.float32(0.25) for c in contours(O)[:m]]
    npts = 1024             # (the sizes of lazily made payloads are fixed numbers: asserted when the payload is made)

    def packed(O):
        pts = np.concatenate(ragged(O))
        assert len(pts) <= npts, len(pts)
        return np.concatenate([pts, np.zeros((npts - len(pts), 2), np.float32)])
    _add("contour_moments_ragged[4 contours,f32]", "va_contour_moments_ragged", NONE,
         [Arg("points", "in", packed, nbytes=npts * 8, itemsize=4),
          Arg("off", "scratch", lambda O: np.concatenate([[0], np.cumsum([len(c) for c in ragged(O)])]).astype(np.int64),
              nbytes=(m + 1) * 8, itemsize=8),
          out("moments", (m, 10), np.float64)],
         lambda L, p, _: L.va_contour_moments_ragged(p["points"], p["off"], m, 1, p["moments"], P.ON.stream),
         lambda O: {"moments": moments(O, ragged(O))})


_contour_moment_cases()


def _simplify_cases():
    import simplify_checks as K
    curves = [np.ascontiguousarray(c, np.float64).reshape(-1, 2) for c in K.random_curves(17, 6, 3, 40)]
    m = len(curves)
    off = np.concatenate([[0], np.cumsum([len(c) for c in curves])]).astype(np.int64)
    npoints = int(off[-1])
    points = np.concatenate(curves)
    tol = np.full(m, 2.0)
    args = [Arg("points", "in", points), Arg("off", "scratch", off), Arg("tol", "scratch", tol),
            out("keep", (npoints,), np.uint8), out("count", (m,), np.int32), out("status", (m,), np.int32)]

    def ref(keep_of):
        flags = [np.asarray(keep_of(c), np.uint8) for c in curves]
        return {"keep": np.concatenate(flags), "count": np.array([int(f.sum()) for f in flags], np.int32),
                "status": np.zeros(m, np.int32)}
    _add("simplify_rdp[6 curves]", "va_simplify_rdp", NONE, args,
         lambda L, p, _: L.va_simplify_rdp(p["points"], p["off"], npoints, m, p["tol"], p["keep"], p["count"], p["status"],
                                           P.ON.stream),
         lambda O: ref(lambda c: K.rdp_keep(c, 2.0)))
    for closed in (0, 1):
        _add("simplify_visvalingam[6 curves,closed%d]" % closed,
             ("va_simplify_visvalingam", "va_simplify_visvalingam_workspace_bytes"), NONE,
             args + [Arg("ws", "scratch", nbytes=lambda L: L.va_simplify_visvalingam_workspace_bytes(npoints))],
             lambda L, p, _, closed=closed: L.va_simplify_visvalingam(
                 p["points"], p["off"], npoints, m, p["tol"], closed, p["keep"], p["count"], p["status"], p["ws"],
                 L.va_simplify_visvalingam_workspace_bytes(npoints), P.ON.stream),
             lambda O, closed=closed: ref(lambda c: K.visvalingam_keep(c, 2.0, bool(closed))))


_simplify_cases()


def _curve_cases():
    import curves_checks as K
    curves = [np.ascontiguousarray(c, np.float64) for c in K.mixed_curves(31, 6, 2, 60)]
    m = len(curves)
    off = np.concatenate([[0], np.cumsum([len(c) for c in curves])]).astype(np.int64)
    spacing, counts = np.full(m, 2.5), np.zeros(m, np.int32)

    def want():
        from video import ops
        from video.analysis import curves as A
        if ops.host_norm_is_pinned():
            return [np.asarray(A.make_curve_equidistant(c, spacing=2.5), np.float64) for c in curves]
        return [K.equidistant(c, spacing=2.5) for c in curves]
    cap = 1024                                                # (asserted: room for every resampled point)

    def ref(O):
        from video.analysis import curves as A
        res = want()
        total = sum(len(r) for r in res)
        assert 0 < total <= cap
        pts = np.zeros((cap, 2))
        pts[:total] = np.concatenate(res)
        return {"count": np.array([len(r) for r in res], np.int32),
                "out_off": np.concatenate([[0], np.cumsum([len(r) for r in res])]).astype(np.int64),
                "in_len": np.array([A.curve_length(c) for c in curves]), "status": np.zeros(m, np.int32),
                "total": np.array([total], np.int64), "pts": pts, "out_len": np.array([A.curve_length(r) for r in res])}
    _add("curves_equidistant[6 curves]", "va_curves_equidistant", NONE,
         [Arg("points", "in", np.concatenate(curves)), Arg("off", "scratch", off), Arg("spacing", "scratch", spacing),
          Arg("counts", "scratch", counts), out("count", (m,), np.int32), out("out_off", (m + 1,), np.int64),
          out("in_len", (m,), np.float64), out("status", (m,), np.int32), out("total", (1,), np.int64),
          out("pts", (cap, 2), np.float64), out("out_len", (m,), np.float64)],
         lambda L, p, _: L.va_curves_equidistant(p["points"], p["off"], int(off[-1]), m, p["spacing"], p["counts"], None,
                                                 p["count"], p["out_off"], p["in_len"], p["status"], p["total"], p["pts"],
                                                 cap, p["out_len"], P.ON.stream),
         ref, project={"pts": lambda a, r: a[:int(r["total"][0])]})


_curve_cases()


def _outline_cases():
    from outline_checks import G
    rng = np.random.default_rng(19)
    outlines = [G.star_ring(rng, k) for k in (5, 9, 17)]
    closed = np.array([1, 1, 0], np.uint8)
    off = np.cumsum([0] + [len(o) for o in outlines]).astype(np.int64)
    pts = np.concatenate(outlines).astype(np.float64)
    q = 24
    ang = rng.uniform(0, 2 * np.pi, q)
    a = np.array([50.0, 50.0]) + rng.uniform(-3, 3, (q, 2))
    f = a + 1000 * np.stack([np.cos(ang), np.sin(ang)], 1)
    index = (np.arange(q) % 3).astype(np.int32)
    xy = np.array([50.0, 50.0]) + rng.uniform(-40, 40, (q, 2))
    for lanes in (8, 64):
        def rays(O):
            t, h, e, c = G.ray_hits(outlines, closed.astype(bool), a, f, index)
            return {"t": np.asarray(t, np.float64), "hit": np.asarray(h, np.float64), "edge": np.asarray(e, np.int32),
                    "count": np.asarray(c, np.int32)}
        _add("ray_hits[3 outlines,lanes%d]" % lanes, "va_ray_hits", NONE,
             [Arg("points", "in", pts), Arg("off", "scratch", off), Arg("closed", "scratch", closed), Arg("a", "in", a),
              Arg("f", "in", f), Arg("index", "scratch", index), out("t", (q,), np.float64), out("hit", (q, 2), np.float64),
              out("edge", (q,), np.int32), out("count", (q,), np.int32)],
             lambda L, p, _, lanes=lanes: L.va_ray_hits(p["points"], p["off"], p["closed"], len(pts), 3, p["a"], p["f"],
                                                        p["index"], q, lanes, p["t"], p["hit"], p["edge"], p["count"],
                                                        P.ON.stream),
             rays)
        _add("points_in_outlines[3 outlines,lanes%d]" % lanes, "va_points_in_outlines", NONE,
             [Arg("points", "in", pts), Arg("off", "scratch", off), Arg("xy", "in", xy), Arg("index", "scratch", index),
              out("inside", (q,), np.uint8)],
             lambda L, p, _, lanes=lanes: L.va_points_in_outlines(p["points"], p["off"], len(pts), 3, p["xy"], p["index"], q,
                                                                  lanes, p["inside"], P.ON.stream),
             lambda O: {"inside": G.contains_points(outlines, xy, index).astype(np.uint8)})


_outline_cases()


def _geodesic_path_case():
    geo = np.load(os.path.join(ROOT, "tests", "golden", "geodesic_v1.npz"), allow_pickle=False)
    names = [n for n in geo["names"] if tuple(geo[n + "/path_end"]) != (-1, -1) and len(geo[n + "/path"]) >= 4
             and min(geo[n + "/map"].shape) >= 8]
    name = sorted(names, key=lambda n: geo[n + "/map"].size)[0]
    dmap = np.ascontiguousarray(geo[name + "/map"], np.int32)
    h, w = dmap.shape
    path = np.asarray(geo[name + "/path"], np.int32).reshape(-1, 2)
    cap = len(path) + 4
    padded = np.zeros((1, cap, 2), np.int32)
    padded[0, :len(path)] = path
    _add("distance_map_path[%s]" % name, ("va_distance_map_path", "va_geodesic_workspace_bytes"), NONE,
         [Arg("map", "in", dmap[None]), Arg("end", "scratch", np.asarray(geo[name + "/path_end"], np.int32).reshape(1, 2)),
          out("path", (1, cap, 2), np.int32), out("npath", (1,), np.int32),
          Arg("ws", "scratch", nbytes=lambda L: L.va_geodesic_workspace_bytes(1, h, w))],
         lambda L, p, _: L.va_distance_map_path(p["map"], 1, h, w, p["end"], p["path"], cap, p["npath"], p["ws"],
                                                L.va_geodesic_workspace_bytes(1, h, w), P.ON.stream),
         lambda O: {"path": padded, "npath": np.array([len(path)], np.int32)},
         project={"path": lambda a, r: a[0, :int(r["npath"][0])]})


_geodesic_path_case()


def _active_contour_cases():
    AG, PG = P.generator("make_golden_active_contour"), P.generator("make_golden_polygon")
    gamma, max_it = 0.1, 12
    planes, curves, mats = [], [], []
    for k, (h, w, N) in enumerate(((24, 32, 12), (10, 12, 7))):
        x = AG.sobel_input(h, w, np.float32, salt=5 + k)
        fx, fy = AG.sobel5(x[None])
        planes.append((np.ascontiguousarray(fx[0], np.float64), np.ascontiguousarray(fy[0], np.float64)))
        t = np.linspace(0.3, 5.5, N)
        curves.append(np.stack([w / 2.0 + w / 3.5 * np.cos(t), h / 2.0 + h / 3.5 * np.sin(t)], 1))
        ds = float(np.hypot(*np.diff(curves[-1], axis=0).T).mean())
        mats.append(PG.evolution_matrix(N, ds, 1.0, 1.0, gamma))

    def snakes(which):
        cap = max(len(curves[k]) for k in which)
        pts = np.zeros((len(which), cap, 2))
        want = {"pts": pts.copy(), "iterations": np.zeros(len(which), np.int32), "tv": np.zeros(len(which))}
        for j, k in enumerate(which):
            pts[j, :len(curves[k])] = curves[k]
            q, it, tv, _ = AG.snake(planes[k][0], planes[k][1], curves[k], mats[k], gamma, 0.0, max_it)
            want["pts"][j, :len(q)], want["iterations"][j], want["tv"][j] = q, it, tv
        flat = np.concatenate([np.ascontiguousarray(mats[k].T).reshape(-1) for k in which])
        moff = np.concatenate([[0], np.cumsum([mats[k].size for k in which])[:-1]]).astype(np.int64)
        return pts, cap, flat, moff, np.array([len(curves[k]) for k in which], np.int32), want

    def common(pts, flat, moff, npts, m):
        return [Arg("npts", "scratch", npts), Arg("mats", "scratch", flat), Arg("mat_off", "scratch", moff),
                Arg("pts", "inout", pts), out("iterations", (m,), np.int32), out("tv", (m,), np.float64)]
    # one contour on one frame
    pts, cap, flat, moff, npts, want = snakes([0])
    h, w = planes[0][0].shape
    _add("active_contour[24x32,12 points]", "va_active_contour", NONE,
         [Arg("fx", "in", planes[0][0][None]), Arg("fy", "in", planes[0][1][None]),
          Arg("frame", "scratch", np.zeros(1, np.int32))] + common(pts, flat, moff, npts, 1),
         lambda L, p, _, h=h, w=w, cap=cap, nm=flat.size: L.va_active_contour(
             p["fx"], p["fy"], 1, h, w, 1, cap, p["npts"], p["frame"], p["mats"], p["mat_off"], nm, None, None, gamma, 0.0,
             max_it, p["pts"], p["iterations"], p["tv"], P.ON.stream),
         lambda O, want=want: want)
    # two contours on two items of different sizes
    pts, cap, flat, moff, npts, want = snakes([0, 1])
    shapes = np.array([q[0].shape for q in planes], np.int32)
    sizes = shapes.prod(axis=1)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    total = int(sizes.sum())
    _add("active_contour_ragged[2 items]", "va_active_contour_ragged", NONE,
         [Arg("fx", "in", np.concatenate([q[0].ravel() for q in planes])),
          Arg("fy", "in", np.concatenate([q[1].ravel() for q in planes])), Arg("shapes", "scratch", shapes),
          Arg("offsets", "scratch", offsets), Arg("item", "scratch", np.arange(2, dtype=np.int32))]
         + common(pts, flat, moff, npts, 2),
         lambda L, p, _, cap=cap, nm=flat.size: L.va_active_contour_ragged(
             p["fx"], p["fy"], p["shapes"], p["offsets"], total, 2, 2, cap, p["npts"], p["item"], p["mats"], p["mat_off"],
             nm, None, None, gamma, 0.0, max_it, p["pts"], p["iterations"], p["tv"], P.ON.stream),
         lambda O, want=want: want)


_active_contour_cases()


def _draw_contours_case():
    import composer_checks as K
    from video import ops
    # three hand-made closed contours on two frames, in the layout va_find_contours writes
    contours = [(0, [(3, 2), (40, 2), (40, 12), (3, 12)]), (0, [(50, 5), (66, 9), (55, 15)]), (1, [(10, 1), (30, 14), (5, 8)])]
    info = np.zeros(len(contours), ops.CONTOUR_INFO_DTYPE)
    info["frame"], info["npoints"] = [f for f, _ in contours], [len(c) for _, c in contours]
    off = np.concatenate([[0], np.cumsum(info["npoints"])]).astype(np.int64)
    points = np.array([p for _, c in contours for p in c], np.int32)
    for c in (1, 3):
        frames = P._u8(1770 + c, 2, 17, 70, c) if c == 3 else P._u8(1770 + c, 2, 17, 70)
        color = 200 if c == 1 else (10, 200, 90)
        packed = color if c == 1 else color[0] | color[1] << 8 | color[2] << 16

        def ref(O, frames=frames, color=color):
            want = frames.copy()
            for f, pts in contours:
                for a, b in zip(pts, pts[1:] + pts[:1]):
                    for x, y in K.line_pixels(70, 17, *a, *b):
                        want[f, y, x] = color
            return {"frames": want, "status": np.zeros(1, np.int32)}
        _add("draw_contours_u8[c%d]" % c, "va_draw_contours_u8", NONE,
             [Arg("frames", "inout", frames), Arg("info", "scratch", info.view(np.uint8)), Arg("off", "scratch", off),
              Arg("points", "scratch", points), out("status", (1,), np.int32)],
             lambda L, p, _, c=c, packed=packed: L.va_draw_contours_u8(
                 p["frames"], 2, 17, 70, c, p["info"], p["off"], len(contours), p["points"], len(points), None, 2, packed,
                 p["status"], P.ON.stream),
             ref)


_draw_contours_case()


def _jpeg_extra_cases():
    import jpeg_decode_checks as D
    import jpeg_optimize_checks as JO
    import jpeg_split_checks as JS
    import jpeg_subsampled_checks as SS
    from video import ops
    # optimal tables of chosen counts: a DC shape, zeros, large counts
    rng = np.random.default_rng(31)
    freq = rng.integers(0, 1000, (4, 256)).astype(np.int64)
    freq[0, 12:] = 0
    freq[1][rng.random(256) < 0.5] = 0
    freq[2] *= 1 << 20
    _add("jpeg_optimal_tables[4 tables]", "va_jpeg_optimal_tables", NONE,
         [Arg("freq", "in", freq), out("tables", (4, JO.TABLE_BYTES), np.uint8)],
         lambda L, p, _: L.va_jpeg_optimal_tables(p["freq"], 4, p["tables"], P.ON.stream),
         lambda O: {"tables": np.stack([JO.table_bytes(*JO.gen_optimal_table(f)) for f in freq])})
    # the optimised encoder at 4:2:0 and on monochrome frames
    for layout, hv in (("420", (2, 2)), ("mono", None)):
        c = 1 if hv is None else 3
        stack = JO.stack_of(3, 16, 24, c, 16024)             # a constant frame, noise, a ramp
        files, tables = JO.encode(stack, 90, hv)
        blob = np.frombuffer(b"".join(bytes(f) for f in files), np.uint8)
        file_off = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)
        pre, post = ops.jpeg_header_pieces(ops.jpeg_header(16, 24, c, 90, hv or (1, 1)))
        nt = 2 if c == 1 else 4
        _add("jpeg_encode_optimized_u8[3x16x24,%s]" % layout, "va_jpeg_encode_optimized_u8", NONE,
             [Arg("frames", "in", stack), Arg("qtables", "in", np.concatenate(ops.jpeg_tables(90))),
              Arg("pre", "in", np.frombuffer(pre, np.uint8)), Arg("post", "in", np.frombuffer(post, np.uint8)),
              out("tables", (nt * JO.TABLE_BYTES,), np.uint8), out("sizes", (3,), np.int64), out("offsets", (4,), np.int64),
              out("totals", (1,), np.int64), out("bytes", (len(blob),), np.uint8)],
             lambda L, p, _, c=c, hv=hv or (1, 1), npre=len(pre), npost=len(post), cap=len(blob): L.va_jpeg_encode_optimized_u8(
                 p["frames"], 3, 16, 24, c, hv[0], hv[1], p["qtables"], p["pre"], npre, p["post"], npost, p["tables"],
                 p["sizes"], p["offsets"], p["totals"], p["bytes"], cap, P.ON.stream),
             lambda O, tables=tables, file_off=file_off, blob=blob: {
                 "tables": np.asarray(tables, np.uint8).ravel(), "sizes": np.diff(file_off), "offsets": file_off,
                 "totals": file_off[-1:], "bytes": blob})
    # the split decoder on two 64 x 48 frames without restart markers
    sub = 48
    datas = [JS.encode_plain(JS.picture(48, 64, seed), "420") for seed in (5, 6)]
    heads = [D.parse_header(d, sampling="any") for d in datas]
    head = heads[0]
    n, h, w, c = 2, head["h"], head["w"], head["c"]
    lh, lv = head["sampling"]
    huff = np.frombuffer(b"".join(ops._jpeg_decode_table(*dc) + ops._jpeg_decode_table(*ac) for dc, ac in head["huff"]),
                         np.uint8)
    segs = [JS.Segment(d, hd) for d, hd in zip(datas, heads)]
    max_scan = max(s.e - s.b for s in segs)
    max_rounds = max(s.lanes(sub) for s in segs)
    file_off = np.concatenate([[0], np.cumsum([len(d) for d in datas])]).astype(np.int64)
    size = lambda L: L.va_jpeg_decode_split_workspace_bytes(n, h, w, c, lh, lv, sub, max_scan)      # noqa: E731
    _add("jpeg_decode_split_u8[2x48x64,4:2:0]", ("va_jpeg_decode_split_u8", "va_jpeg_decode_split_workspace_bytes"), NONE,
         [Arg("bytes", "in", np.frombuffer(b"".join(datas), np.uint8), decoy=False), Arg("offsets", "scratch", file_off),
          Arg("scan_begin", "scratch", np.array([hd["scan_begin"] for hd in heads], np.int64)),
          Arg("qtables", "in", np.ascontiguousarray(head["qtables"]).ravel(),       # (quality 100: all ones)
              decoy=np.ascontiguousarray(head["qtables"]).ravel() * 2), Arg("huff", "scratch", huff),
          out("frames", (n, h, w, c), np.uint8), out("status", (n,), np.int32), out("rounds", (n,), np.int32),
          Arg("ws", "scratch", nbytes=size)],
         lambda L, p, _: L.va_jpeg_decode_split_u8(
             p["bytes"], p["offsets"], p["scan_begin"], n, h, w, c, lh, lv, p["qtables"], p["huff"], len(huff), p["frames"],
             p["status"], p["ws"], size(L), sub, max_rounds, max_scan, p["rounds"], P.ON.stream),
         lambda O: {"frames": np.stack([SS.decode(d, hd)[0] for d, hd in zip(datas, heads)]),
                    "status": np.zeros(n, np.int32),
                    "rounds": np.array([JS.scan(s, sub)[0] for s in segs], np.int32)})


_jpeg_extra_cases()


def _overlapped_pipeline_cases():
    """va_pipeline_overlap(p, 1): the paint of the label image runs on the pipeline's own non-blocking stream, behind an
    event of the caller's stream, and labels_out is complete on a stream only behind va_pipeline_fence.  (The table's
    pipeline cases leave the overlap off: nothing of theirs runs on the side stream and their fence finds nothing to
    wait for.  These cannot be in that table: its runner reads the outputs back without a fence.)"""
    for shape, background, family in (((2, 32, 64), True, "mfma-i8"), ((2, 32, 64), False, "mfma-i8"),
                                      ((2, 33, 70), True, "mfma-i8-planes")):
        n, h, w = shape
        clip = P.pipeline_clip(n, h, w)
        thresh = P.PIPELINE_THRESH[background]

        def setup(L, w=w, h=h, n=n, background=background, thresh=thresh, family=family):
            p = P.make_pipeline(L, w, h, n, background, 1.0, thresh, True, 4)
            assert ("gauss=%s(" % family).encode() in L.va_pipeline_describe(p), L.va_pipeline_describe(p)
            assert L.va_pipeline_overlap(p, 1) == 0, L.va_last_error()
            return p

        def prepare(L, p, background=background):
            if background:
                assert L.va_bg_set_state(p, None, 0, 0) == 0              # every run starts a fresh model

        def ref(O, clip=clip, background=background, thresh=thresh):
            r = P.chain_reference(O, clip, background, 1.0, thresh, True, 4)
            return {k: r[k] for k in ("mask", "labels", "counts")}
        _add("pipeline_overlapped[%dx%d,%s,close,ccl4]" % (h, w, "mean" if background else "none"),
             ("va_pipeline_create", "va_pipeline_overlap", "va_pipeline_run", "va_pipeline_fence", "va_pipeline_describe",
              "va_bg_set_state"), NONE,
             [Arg("frames", "in", clip, decoy=np.repeat(clip[:1], n, 0) if background else None),
              out("mask", shape, np.uint8), out("labels", shape, np.int32),
              out("counts", (n,), np.int32)],
             lambda L, ptr, p, n=n: L.va_pipeline_run(p, ptr["frames"], n, None, ptr["mask"], ptr["labels"], ptr["counts"],
                                                      None, P.ON.stream),
             ref, setup=setup, teardown=lambda L, p: p is not None and L.va_pipeline_destroy(p), prepare=prepare,
             rejoin=lambda L, p, stream: L.va_pipeline_fence(p, stream))


_overlapped_pipeline_cases()

CASES = list(P.CASES) + EXTRA
BY_NAME = {c.name: c for c in CASES}
# the case that runs between the plain and the gated run of every other case: other sizes of leased scratch
INTERLOPERS = ("gaussian_u8[2x33x70x3,s1]", "morph_bits_u8[dilate,w70]")
SENSITIVITY = ("threshold_u8[4096]", "gaussian_u8_generic[2x33x70]", "morph_u8[dilate,rect5,w64]")


# ---------------------------------------------------------------------------------------------- the runner
class Device(object):
    """a va_malloc block of nbytes (and a little more, so that no allocation is empty)"""

    def __init__(self, be, nbytes):
        self.be, self.nbytes, self.ptr = be, int(nbytes), C.c_void_p()
        be.check(be.lib.va_malloc(C.byref(self.ptr), self.nbytes + P.PAD))

    def upload(self, array):
        array = np.ascontiguousarray(array)
        assert array.nbytes == self.nbytes, (array.nbytes, self.nbytes)
        if array.nbytes:
            self.be.check(self.be.lib.va_memcpy_h2d(self.ptr, array.ctypes.data, array.nbytes, None))

    def fill(self, byte):
        self.be.check(self.be.lib.va_memset(self.ptr, byte, self.nbytes + P.PAD, None))

    def download(self):
        got = np.empty(self.nbytes, np.uint8)
        if got.nbytes:
            self.be.check(self.be.lib.va_memcpy_d2h(got.ctypes.data, self.ptr, got.nbytes, None))
        return got

    def free(self):
        if self.ptr.value:
            self.be.lib.va_free(self.ptr)
            self.ptr = C.c_void_p()


class Blocker(object):
    """product calls on buffers of its own that keep a stream busy: REPS generic Gaussians of 6 x 301 x 517 at a
    sigma of 30 (181 taps: the host enqueues a launch much faster than the GPU runs it).  DESIGN.md, "Stream order",
    has the measured times that size it."""
    SHAPE, SIGMA, REPS = (6, 301, 517), 30.0, 192

    def __init__(self, be, reps=None):
        self.be, self.reps = be, reps or self.REPS
        size = int(np.prod(self.SHAPE))
        self.src, self.dst = Device(be, size), Device(be, size)
        self.src.upload(np.random.default_rng(321).integers(0, 256, self.SHAPE, dtype=np.uint8))
        be.check(be.lib.va_stream_sync(None))

    def enqueue(self, stream):
        n, h, w = self.SHAPE
        for _ in range(self.reps):
            self.be.check(self.be.lib.va_gaussian_u8_generic(self.src.ptr, self.dst.ptr, n, h, w, 1, self.SIGMA, stream))

    def free(self):
        self.src.free()
        self.dst.free()


class Run(object):
    """the buffers of one case on one backend: working, staging, decoy and keep copies"""

    def __init__(self, be, case, oracle):
        L = be.lib
        assert case.runs_on(L), case
        self.be, self.case, self.ctx = be, case, None
        self.work, self.stage, self.decoy_dev, self.keep, self.decoys = {}, {}, {}, {}, {}
        self.made_ctx = False
        for a in case.args:
            a.resolve(oracle)
            self.work[a.name] = Device(be, a.nbytes(L))
            d = a.decoy()
            if d is not None:
                self.decoys[a.name] = d
                self.stage[a.name], self.decoy_dev[a.name] = Device(be, d.nbytes), Device(be, d.nbytes)
            if a.role in ("out", "inout"):
                self.keep[a.name] = Device(be, a.nbytes(L))
        self.ptr = {name: dev.ptr.value for name, dev in self.work.items()}

    def setup(self):
        if self.case.setup and not self.made_ctx:
            self.ctx = self.case.setup(self.be.lib)
        self.made_ctx = True

    def free(self):
        if self.case.teardown and self.made_ctx:
            self.case.teardown(self.be.lib, self.ctx)
        self.made_ctx = False
        for group in (self.work, self.stage, self.decoy_dev, self.keep):
            for dev in group.values():
                dev.free()

    # inputs: "true" (the case's payloads) or "decoy" (the decoys where there are any)
    def load(self, which):
        for a in self.case.args:
            dev = self.work[a.name]
            if a.role == "out" or not isinstance(a.array, np.ndarray):
                dev.fill(SENTINEL)
            else:
                dev.upload(self.decoys[a.name] if which == "decoy" and a.name in self.decoys else a.array)
        self.be.check(self.be.lib.va_stream_sync(None))

    def call(self, stream):
        P.ON.stream = stream
        try:
            if self.case.prepare:
                self.case.prepare(self.be.lib, self.ctx)
            return self.case.call(self.be.lib, self.ptr, self.ctx)
        finally:
            P.ON.stream = None

    def outputs(self, group):
        return {a.name: group[a.name].download() for a in self.case.args if a.role in ("out", "inout")}


def mismatches(case, refs, got):
    """the outputs that differ from the reference (projected as the case says): [(name, elements)]"""
    bad = []
    for a in case.args:
        if a.role in ("out", "inout"):
            want = refs[a.name]
            g = got[a.name].view(want.dtype).reshape(want.shape)
            if a.name in case.project:
                g, want = case.project[a.name](g, refs), case.project[a.name](want, refs)
            g, want = np.ascontiguousarray(g), np.ascontiguousarray(want)
            if g.tobytes() != want.tobytes():
                bad.append((a.name, int(np.count_nonzero(g.view(np.uint8) != want.view(np.uint8)))))
    return bad


def references(run, oracle):
    case = run.case
    if getattr(case, "self_reference", False):
        if case.name not in P._REFS:                         # its own output on the null stream
            run.load("true")
            run.be.check(run.call(None))
            run.be.check(run.be.lib.va_stream_sync(None))
            got = run.outputs(run.work)
            P._REFS[case.name] = {a.name: got[a.name].view(np.dtype("u1")) for a in case.args if a.role == "out"}
        return P._REFS[case.name]
    return P.reference(case, oracle)


def run_plain(run, oracle, stream, compare=True):
    """inputs in place and synchronised, the call on `stream`, one synchronisation, every output compared"""
    be, L = run.be, run.be.lib
    refs = references(run, oracle)
    run.load("true")
    rc = run.call(stream)
    assert rc == 0, (run.case, "plain", rc, L.va_last_error())
    if run.case.rejoin:
        be.check(run.case.rejoin(L, run.ctx, stream))
    if not compare:
        return
    be.check(L.va_stream_sync(stream))
    bad = mismatches(run.case, refs, run.outputs(run.work))
    assert not bad, (run.case, "plain run on a created stream", bad)


def run_gated(run, oracle, stream, blocker, events, call_stream="same"):
    """the gated run; returns (the outputs that differ from the reference, the call's span t1 - t0 in seconds, the
    blocker's time D in seconds).  call_stream: the stream handed to the entry point ("same": `stream`)."""
    be, L, case = run.be, run.be.lib, run.case
    refs = references(run, oracle)
    run.load("decoy")
    for name, decoy in run.decoys.items():
        arg = next(a for a in case.args if a.name == name)
        run.stage[name].upload(arg.array)
        run.decoy_dev[name].upload(decoy)
    for dev in run.keep.values():
        dev.fill(SENTINEL)
    if case.prepare:                                        # (may synchronise: in front of the blocker)
        case.prepare(L, run.ctx)
    be.check(L.va_stream_sync(None))
    be.check(L.va_stream_sync(stream))
    e0, e1 = events
    t0 = time.perf_counter()
    be.check(L.va_event_record(e0, stream))
    blocker.enqueue(stream)
    be.check(L.va_event_record(e1, stream))
    for name in run.decoys:
        be.check(L.va_memcpy_d2d(run.work[name].ptr, run.stage[name].ptr, run.stage[name].nbytes, stream))
    P.ON.stream = stream if call_stream == "same" else call_stream
    try:
        rc = case.call(L, run.ptr, run.ctx)
    finally:
        P.ON.stream = None
    t1 = time.perf_counter()
    assert rc == 0, (case, "gated", rc, L.va_last_error())
    if case.rejoin:
        be.check(case.rejoin(L, run.ctx, stream))
    for name, dev in run.keep.items():
        be.check(L.va_memcpy_d2d(dev.ptr, run.work[name].ptr, dev.nbytes, stream))
    for name in run.decoys:
        be.check(L.va_memcpy_d2d(run.work[name].ptr, run.decoy_dev[name].ptr, run.decoy_dev[name].nbytes, stream))
    be.check(L.va_stream_sync(stream))
    be.check(L.va_stream_sync(None))
    ms = C.c_float()
    be.check(L.va_event_elapsed_ms(e0, e1, C.byref(ms)))
    return mismatches(case, refs, run.outputs(run.keep)), t1 - t0, ms.value / 1e3


def constant(array):
    """one value repeated (or nothing at all)"""
    flat = np.ascontiguousarray(array).reshape(-1)
    return flat.size == 0 or bool(np.all(flat == flat[0]))


def decoy_distinguishes(run, oracle):
    """one unblocked run on the decoys, on the null stream: the decoy is a valid input (the call returns 0) and its
    result differs from the true one in every output that can tell inputs apart -- an output whose reference is one
    repeated value (a status of zeros) cannot -- so that a misordered run cannot give the reference's bytes by accident.
    A case without inputs has no decoy and is exempt (it can show a hidden synchronisation only)."""
    be, L, case = run.be, run.be.lib, run.case
    if not run.decoys:
        return
    refs = references(run, oracle)
    run.load("decoy")
    rc = run.call(None)
    assert rc == 0, (case, "the decoy is not a valid input", rc, L.va_last_error())
    if case.rejoin:
        be.check(case.rejoin(L, run.ctx, None))
    be.check(L.va_stream_sync(None))
    differing = {name for name, _ in mismatches(case, refs, run.outputs(run.work))}
    telling = {a.name for a in case.args if a.role in ("out", "inout") and a.name not in DECOY_BLIND.get(case.name, ())
               and not constant(case.project[a.name](refs[a.name], refs) if a.name in case.project else refs[a.name])}
    assert telling, (case, "no output can tell the decoy from the true input")
    assert telling <= differing, (case, "the decoy's result equals the true one in", sorted(telling - differing))


def run_case(be, case, oracle, stream, blocker, events, interloper=None):
    """plain, (the interloper, unsynchronised,) gated, gated under the zero fill; returns [(mode, span, D)]"""
    from video import _hip
    L = be.lib
    run = Run(be, case, oracle)
    figures = []
    try:
        run.setup()
        run_plain(run, oracle, stream)
        decoy_distinguishes(run, oracle)
        if interloper is not None:
            run_plain(interloper, oracle, stream, compare=False)
        for mode, fill in (("gated", None), ("gated+fill", 0)):
            if fill is not None:
                be.check(L.va_test_hook_fill(fill))
            try:
                bad, span, busy = run_gated(run, oracle, stream, blocker, events)
            finally:
                if fill is not None:
                    be.check(L.va_test_hook_fill(_hip.fill_mode()))
            figures.append((mode, span, busy))
            covered = span < busy
            if not synchronises(case):
                assert covered, ("%s, %s: the call returned %.2f ms after the blocker was enqueued, and the blocker kept "
                                 "the stream busy for %.2f ms: the call synchronised, or the blocker is too short"
                                 % (case, mode, span * 1e3, busy * 1e3))
            elif case.name not in NOTHING_TO_WAIT_FOR:
                assert not covered, ("%s, %s: declared `synchronises`, but the call returned after %.2f ms while the "
                                     "blocker held the stream for %.2f ms" % (case, mode, span * 1e3, busy * 1e3))
            assert not bad, (case, mode, "covered" if covered else "not covered", bad)
    finally:
        be.lib.va_stream_sync(stream)
        run.free()
    return figures
