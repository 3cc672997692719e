"""GPU: skeleton graphs (va_skeleton_graph, ops.skeleton_graphs, ops.polygon_skeleton_graphs), MorphologicalGraph
and Polygon.get_morphological_graph against the restatement of the pinned definition in
tests/golden/make_golden_skeleton_graph.py.  Every array is compared with np.array_equal.  Reads the generators'
restatements and tables only."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_skeleton_graph", os.path.join(ROOT, "tests", "golden", "make_golden_skeleton_graph.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()


def _restate(img):
    if img.size == 0:
        return np.zeros((0, 4), np.int32), np.zeros((0, 3), np.int32), np.zeros(0), []
    return G.skeleton_graph(img)


@pytest.fixture(scope="module")
def batch():
    """(names, images, restated graphs) of the ragged batch of case 1, computed once"""
    from video import _hip
    _hip.lib()
    rng = np.random.default_rng(3)
    cases = list(G.all_cases().items())                                  # hand cases and fixture skeletons
    cases += [("ones%dx%d" % s, np.ones(s, np.uint8)) for s in ((1, 1), (1, 9), (9, 1), (2, 2))]
    cases.append(("empty_item", np.zeros((0, 7), np.uint8)))
    cases.append(("no_foreground", np.zeros((6, 7), np.uint8)))
    cases += [("full_33x64", np.ones((33, 64), np.uint8)), ("full_40x65", np.ones((40, 65), np.uint8))]
    cases += G.border_items()                                            # widths 1 .. 70, one after the other
    skel = dict(cases)["skel/blob3"]
    cases.append(("odd_1x3", np.ones((1, 3), np.uint8)))                 # the items after it lie at odd offsets
    cases.append(("v255", skel * np.uint8(255)))
    cases.append(("mixed", skel * rng.integers(1, 256, skel.shape).astype(np.uint8)))
    cases.append(("bool", skel.astype(bool)))
    names, imgs = [n for n, _ in cases], [m for _, m in cases]
    return names, imgs, [_restate(np.asarray(m)) for m in imgs]


def _same(got, want, name):
    nodes, edges, lengths, curves = want
    assert got.nodes.dtype.names == ("item", "x", "y", "degree", "pixels"), name
    assert np.array_equal(np.c_[got.nodes["x"], got.nodes["y"], got.nodes["degree"], got.nodes["pixels"]].reshape(-1, 4),
                          nodes), name
    assert np.array_equal(np.c_[got.edges["node_a"], got.edges["node_b"], got.edges["npoints"]].reshape(-1, 3),
                          edges), name
    assert got.edges["length"].dtype == np.float64 and np.array_equal(got.edges["length"], lengths), name
    assert len(got.curves) == len(curves), name
    for c, w in zip(got.curves, curves):
        assert c.dtype == np.int32 and np.array_equal(c, w), name


# ----------------------------------------------------------------------------------------- 1: ragged call
def test_ragged_batch_equals_restatement(batch):
    from video import ops
    names, imgs, want = batch
    assert {m.shape[1] for m in imgs} >= set(range(1, 71)) and len(imgs) >= 120
    offsets = np.cumsum([0] + [m.size for m in imgs])
    assert np.any(offsets[:-1] % 2 == 1)
    keep = [np.array(m, copy=True) for m in imgs]
    got = ops.skeleton_graphs(imgs)
    assert len(got) == len(imgs)
    for k, (name, g, w) in enumerate(zip(names, got, want)):
        _same(g, w, name)
        assert np.all(g.nodes["item"] == k) and np.all(g.edges["item"] == k), name
    for name, m, k in zip(names, imgs, keep):                            # the inputs are left alone
        assert np.array_equal(m, k), name
    one = dict(zip(names, got))["full_40x65"]                            # a node set larger than a workgroup
    assert one.nodes["pixels"].tolist() == [40 * 65 - 4] and len(one.edges) == 4


def test_each_item_alone_equals_batched(batch):
    from video import ops
    names, imgs, want = batch
    for name, m, w in zip(names, imgs, want):
        _same(ops.skeleton_graphs([m])[0], w, name)
    _same(ops.skeleton_graphs(np.asarray(imgs[names.index("hand/cross_x")])), want[names.index("hand/cross_x")], "2-d")
    assert ops.skeleton_graphs([]) == []
    with pytest.raises(TypeError):
        ops.skeleton_graphs([np.zeros((3, 3), np.float32)])
    with pytest.raises(ValueError):
        ops.skeleton_graphs(np.zeros((2, 2, 2, 2), np.uint8))


# ------------------------------------------------------------------------------- 2: frames, long chains
def test_frame_stack_serpentine_and_nested_rings():
    from video import ops
    T = G.thinning()
    stack = np.stack([T.guo_hall(T.blob(900 + k, 270, 480, 5.0, -0.2))[0] for k in range(2)])
    got = ops.skeleton_graphs(stack)
    assert len(got) == 2
    for k in range(2):
        want = _restate(stack[k])
        assert len(want[0]) > 50 and max(len(c) for c in want[3]) > 32
        _same(got[k], want, "frame%d" % k)
    serp, rings = G.serpentine(64, 64), G.nested_rings(8)
    got = ops.skeleton_graphs([serp, rings])
    want = _restate(serp)
    assert len(want[1]) == 1 and want[1][0, 2] == 32 * 64 + 32
    _same(got[0], want, "serpentine")
    want = _restate(rings)
    assert want[1][:, :2].tolist() == [[k, k] for k in range(8)] and want[0][:, 2].tolist() == [2] * 8
    _same(got[1], want, "rings")


def test_more_scan_workgroups_than_one_round_takes():
    """the scan of the workgroups' sums takes 1024 of them (2^20 pixels) a round: an empty item puts the rings into
    the second round, behind the node, edge and point counts that the serpentine left in the carry"""
    from video import ops
    imgs = [G.serpentine(64, 64), np.zeros((1023, 1024), np.uint8), G.nested_rings(8)]
    assert imgs[0].size + imgs[1].size > 1 << 20
    got = ops.skeleton_graphs(imgs)
    for k, (g, m) in enumerate(zip(got, imgs)):
        _same(g, _restate(m), k)
        assert np.all(g.nodes["item"] == k) and np.all(g.edges["item"] == k), k
    assert len(got[0].edges) == 1 and len(got[2].nodes) == 8


# ---------------------------------------------------------------------------- 3, 4: the C ABI's own rules
def _abi_run(imgs, capn, cape, capp, fill=0xA5):
    """one va_skeleton_graph call into fresh buffers filled with `fill`: (counts, totals, and the raw bytes of the
    node, edge, offset and point buffers, each one record longer than its capacity)"""
    from video import _hip, ops
    L = _hip.lib()
    flat, shapes, offsets, sizes, total = ops._pack_ragged([np.ascontiguousarray(m).view(np.uint8) for m in imgs])
    m = len(imgs)
    nb, eb = ops.SKELETON_NODE_DTYPE.itemsize, ops.SKELETON_EDGE_DTYPE.itemsize
    sizes = {"nodes": (capn + 1) * nb, "edges": (cape + 1) * eb, "off": (cape + 2) * 8, "points": (capp + 1) * 8}
    bufs = {k: _hip.DeviceBuffer.from_array(np.full(v, fill, np.uint8)) for k, v in sizes.items()}
    src, sb, ob = (_hip.DeviceBuffer.from_array(a) for a in (flat, shapes, offsets))
    cnt, tot = _hip.DeviceBuffer(m * 8), _hip.DeviceBuffer(24)
    ws_bytes = L.va_skeleton_graph_workspace_bytes(total, m)
    ws = _hip.DeviceBuffer(ws_bytes)
    _hip.check(L.va_skeleton_graph(src.ptr, sb.ptr, ob.ptr, total, m, cnt.ptr, tot.ptr, bufs["nodes"].ptr, capn,
                                   bufs["edges"].ptr, bufs["off"].ptr, cape, bufs["points"].ptr, capp, ws.ptr,
                                   ws_bytes, None))
    out = {k: b.download((sizes[k],), np.uint8) for k, b in bufs.items()}
    res = cnt.download((m, 2), np.int32), tot.download((3,), np.int64), out
    for b in list(bufs.values()) + [src, sb, ob, cnt, tot, ws]:
        b.free()
    return res


def test_capacities_of_one(batch):
    from video import ops
    names, imgs, want = batch
    true = [sum(len(w[0]) for w in want), sum(len(w[1]) for w in want), sum(int(w[1][:, 2].sum()) for w in want)]
    counts, totals, out = _abi_run(imgs, 1, 1, 1)
    assert totals.tolist() == true                                       # always the true totals
    assert counts.tolist() == [[len(w[0]), len(w[1])] for w in want]
    nb, eb = ops.SKELETON_NODE_DTYPE.itemsize, ops.SKELETON_EDGE_DTYPE.itemsize
    # slot 0 has its records and offsets; its points (3 of them) do not fit and are not written
    node = out["nodes"][:nb].view(ops.SKELETON_NODE_DTYPE)[0]
    first = next(w for w in want if len(w[0]))
    assert [node["x"], node["y"], node["degree"], node["pixels"]] == first[0][0].tolist()
    edge = out["edges"][:eb].view(ops.SKELETON_EDGE_DTYPE)[0]
    first = next(w for w in want if len(w[1]))
    assert [edge["node_a"], edge["node_b"], edge["npoints"]] == first[1][0].tolist() and edge["length"] == first[2][0]
    assert out["off"][:16].view(np.int64).tolist() == [0, int(first[1][0, 2])]
    # nothing is written beyond a capacity
    assert np.all(out["nodes"][nb:] == 0xA5) and np.all(out["edges"][eb:] == 0xA5)
    assert np.all(out["off"][16:] == 0xA5) and np.all(out["points"] == 0xA5)
    # room for exactly the first edge's points: they are written, nothing after them
    counts, totals, out = _abi_run(imgs, 0, 2, int(first[1][0, 2]))
    assert totals.tolist() == true and np.all(out["nodes"] == 0xA5)
    npts = int(first[1][0, 2])
    assert np.array_equal(out["points"][:8 * npts].view(np.int32).reshape(-1, 2), first[3][0])
    assert np.all(out["points"][8 * npts:] == 0xA5) and np.all(out["edges"][2 * eb:] == 0xA5)


def test_wrapper_runs_exactly_once_more_with_exact_room(batch, monkeypatch):
    from video import _hip, ops
    names, imgs, want = batch
    calls = []
    L = _hip.lib()
    real = L.va_skeleton_graph

    class Counting(object):
        def __getattr__(self, name):
            return getattr(L, name)

        def va_skeleton_graph(self, *args):
            calls.append((args[8], args[11], args[13]))
            return real(*args)
    monkeypatch.setattr(_hip, "lib", lambda device=None: Counting())
    monkeypatch.setattr(ops, "DEFAULT_SKELETON_NODE_CAPACITY", 1)
    monkeypatch.setattr(ops, "DEFAULT_SKELETON_EDGE_CAPACITY", 1)
    monkeypatch.setattr(ops, "DEFAULT_SKELETON_POINT_CAPACITY", 1)
    got = ops.skeleton_graphs(imgs)
    true = (sum(len(w[0]) for w in want), sum(len(w[1]) for w in want), sum(int(w[1][:, 2].sum()) for w in want))
    assert calls == [(1, 1, 1), true]
    for name, g, w in zip(names, got, want):
        _same(g, w, name)
    monkeypatch.undo()
    del calls[:]
    monkeypatch.setattr(_hip, "lib", lambda device=None: Counting())
    ops.skeleton_graphs(imgs[:20])
    assert len(calls) == 1                                               # the defaults have room: one run


def test_two_runs_write_identical_bytes(batch):
    names, imgs, want = batch
    a = _abi_run(imgs, 4096, 4096, 1 << 16, fill=0x00)
    b = _abi_run(imgs, 4096, 4096, 1 << 16, fill=0x00)
    assert a[1].tolist() == b[1].tolist() and max(a[1][:2]) <= 4096 and a[1][2] <= 1 << 16
    assert np.array_equal(a[0], b[0])
    for k in a[2]:
        assert np.array_equal(a[2][k], b[2][k]), k


# ------------------------------------------------------------------------------- 5: class and Polygon layer
def _same_graph(g, w, name):
    assert type(g).__name__ == "MorphologicalGraph" and list(g.nodes(data=True)) == list(w.nodes(data=True)), name
    ge, we = list(g.edges(keys=True, data=True)), list(w.edges(keys=True, data=True))
    assert len(ge) == len(we), name
    for (a1, b1, k1, d1), (a2, b2, k2, d2) in zip(ge, we):
        assert (a1, b1, k1) == (a2, b2, k2) and d1["length"] == d2["length"], name
        assert d1["curve"].shape == d2["curve"].shape and np.array_equal(d1["curve"], d2["curve"]), name


def test_from_skeleton_and_from_skeletons(batch):
    from video.analysis.morphological_graph import MorphologicalGraph
    names, imgs, want = batch
    pick = [k for k, n in enumerate(names) if n.startswith(("hand/", "skel/")) and imgs[k].size]
    for post in (False, True):
        graphs = MorphologicalGraph.from_skeletons([imgs[k] for k in pick], post_process=post)
        for k, g in zip(pick, graphs):
            nodes, edges, lengths, curves = want[k]
            _same_graph(g, MorphologicalGraph.from_arrays(nodes, edges, curves, post), names[k])
    for name in ("skel/blob4", "skel/comb7", "hand/ones5x9", "skel/ring3"):
        k = names.index(name)
        nodes, edges, lengths, curves = want[k]
        _same_graph(MorphologicalGraph.from_skeleton(imgs[k]), MorphologicalGraph.from_arrays(nodes, edges, curves),
                    name)
        _same_graph(MorphologicalGraph.from_skeleton(imgs[k], post_process=False),
                    MorphologicalGraph.from_arrays(nodes, edges, curves, False), name)
    stack = np.stack([imgs[names.index("skel/blob0")]] * 2)
    assert len(MorphologicalGraph.from_skeletons(stack)) == 2


def test_polygon_morphological_graphs():
    from video.analysis import shapes
    from video.analysis.morphological_graph import MorphologicalGraph
    T = G.thinning()
    polys = [shapes.Polygon(T.POL.FILL_POLYS[name]) for name in T.POLYGONS]
    singles = []
    for name, poly in zip(T.POLYGONS, polys):
        mask, off = T.POL.get_mask(T.POL.FILL_POLYS[name], 5)
        nodes, edges, lengths, curves = _restate(T.guo_hall(mask)[0])
        want = MorphologicalGraph.from_arrays(nodes, edges, curves)      # from_skeleton of the restated skeleton
        want.simplify(0.1)
        want.translate(*off)
        got = poly.get_morphological_graph()
        _same_graph(got, want, name)
        singles.append(got)
        raw = MorphologicalGraph.from_arrays(nodes, edges, curves)
        raw.translate(*off)
        _same_graph(poly.get_morphological_graph(simplify_epsilon=0), raw, name)
    for eps in (0.1, 0):
        batched = shapes.get_morphological_graphs(polys, simplify_epsilon=eps)
        assert len(batched) == len(polys)
        for name, poly, g in zip(T.POLYGONS, polys, batched):
            _same_graph(g, singles[T.POLYGONS.index(name)] if eps else poly.get_morphological_graph(0), name)
    assert shapes.get_morphological_graphs([]) == []


def test_polygon_batch_with_a_box_above_the_resident_thinning_limit():
    """only the oversized box takes the per-item thinning path; every graph equals the per-op chain's"""
    from video import ops
    T = G.thinning()
    big = np.array([[0, 0], [1100, 40], [1080, 300], [600, 260], [560, 500], [20, 480]], np.int64)
    contours = [np.asarray(T.POL.FILL_POLYS["worm"]).astype(np.int64), big,
                np.asarray(T.POL.FILL_POLYS["star"]).astype(np.int64)]
    boxes = []
    for c in contours:
        x0, y0 = c.min(axis=0) - 5
        x1, y1 = c.max(axis=0) + 5
        boxes.append((x0, y0, x1 - x0, y1 - y0))
    words = [ops._thin_words((b[3], b[2])) for b in boxes]
    assert words[1] > ops.THIN_RESIDENT_MAX_WORDS and max(words[0], words[2]) <= ops.THIN_RESIDENT_MAX_WORDS
    skeletons = ops.guo_hall_thinning(ops.fill_polys(contours, boxes))
    want = ops.skeleton_graphs(skeletons)
    got = ops.polygon_skeleton_graphs(contours, boxes)
    assert len(got) == 3 and len(want[1].edges) > 3
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g.nodes, w.nodes) and np.array_equal(g.edges, w.edges), k
        assert len(g.curves) == len(w.curves) and all(np.array_equal(a, b) for a, b in zip(g.curves, w.curves)), k
    _same(got[0], _restate(skeletons[0]), "worm")
