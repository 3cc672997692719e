"""CPU: the skeleton-graph fixture (tests/golden/skeleton_graph_v1.npz), the restatement of the pinned definition
(tests/golden/make_golden_skeleton_graph.py), curves.simplify_curve / merge_curves and the MorphologicalGraph class
built from the restatement's arrays.  Needs no GPU and no reference checkout."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPZ = os.path.join(ROOT, "tests", "golden", "skeleton_graph_v1.npz")


def _generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_skeleton_graph", os.path.join(ROOT, "tests", "golden", "make_golden_skeleton_graph.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()


@pytest.fixture(scope="module")
def fx():
    return np.load(NPZ, allow_pickle=False)


@pytest.fixture(scope="module")
def restated(fx):
    """name -> (image, skeleton_graph(image, detail=True)) of every image of the fixture, computed once"""
    names = [k[4:] for k in fx.files if k.startswith("img/")]
    return {name: (fx["img/" + name], G.skeleton_graph(fx["img/" + name], detail=True)) for name in names}


def test_fixture_is_complete_and_is_the_restatement(fx, restated):
    assert os.path.getsize(NPZ) < 400 * 1024
    cases = G.all_cases()
    assert sorted(cases) == sorted(restated) and len(cases) == len(G.HAND_CASES) + 30
    for name, img in cases.items():
        assert np.array_equal(img, fx["img/" + name]), name
        nodes, edges, lengths, curves = restated[name][1][:4]
        assert np.array_equal(nodes, fx["nodes/" + name]), name
        assert np.array_equal(edges, fx["edges/" + name]), name
        assert np.array_equal(lengths, fx["lengths/" + name]), name
        assert np.array_equal(np.concatenate(curves + [np.zeros((0, 2), np.int32)]), fx["points/" + name]), name


def test_restatement_gives_the_hand_cases(restated):
    for name, (img, want_nodes, want_edges) in G.HAND_CASES.items():
        got_img, (nodes, edges, lengths, curves, _, _) = restated["hand/" + name]
        assert np.array_equal(got_img, img), name
        assert nodes.tolist() == [list(n) for n in want_nodes], name
        assert len(edges) == len(want_edges), name
        for (a, b, npoints), curve, (wa, wb, pts) in zip(edges.tolist(), curves, want_edges):
            assert (a, b, npoints) == (wa, wb, len(pts)) and curve.tolist() == [list(p) for p in pts], name
    # the L corner is one plain edge, the serpentine one edge, the nested rings two rings
    assert len(restated["hand/corner_l"][1][1]) == 1 and len(restated["hand/serpentine"][1][1]) == 1
    assert restated["hand/nested2"][1][1][:, :2].tolist() == [[0, 0], [1, 1]]
    r2 = G.R2
    assert restated["hand/diag3"][1][2].tolist() == [r2 + r2]
    assert restated["hand/diamond"][1][2].tolist() == [r2 + r2 + r2 + r2]
    assert restated["hand/ring4"][1][2].tolist() == [12.0]


def test_invariants_of_every_fixture_image(restated):
    from video.analysis import curves as C
    for name, (img, (nodes, edges, lengths, curves, sets, chains)) in restated.items():
        # the chain pixels of all edges and the pixels of all node sets partition the foreground
        seen = [p for s in sets for p in s] + [p for c in chains for p in c]
        assert len(seen) == len(set(seen)), name
        ys, xs = np.nonzero(img)
        assert set(seen) == set(zip(xs.tolist(), ys.tolist())), name
        assert [len(s) for s in sets] == nodes[:, 3].tolist(), name
        degree = np.zeros(len(nodes), np.int64)
        for (a, b, npoints), length, curve, chain in zip(edges.tolist(), lengths.tolist(), curves, chains):
            # every edge runs from the anchor of node_a to the anchor of node_b
            assert curve[0].tolist() == nodes[a, :2].tolist() and curve[-1].tolist() == nodes[b, :2].tolist(), name
            assert len(curve) == npoints and 2 + len(chain) <= npoints <= 4 + len(chain) and len(chain) >= 1, name
            assert length == C.curve_length(curve), name
            degree[a] += 1
            degree[b] += 1
        assert degree.tolist() == nodes[:, 2].tolist(), name


def test_m_adjacency_leaves_no_spurious_loops(restated):
    for k in range(8):
        edges = restated["skel/blob%d" % k][1][1]
        assert not np.any(edges[:, 0] == edges[:, 1]), k
    for k in range(4):                                               # each worm skeleton: 2 nodes, 1 edge
        nodes, edges = restated["skel/worm%d" % k][1][:2]
        assert len(nodes) == 2 and len(edges) == 1 and nodes[:, 2].tolist() == [1, 1], k


def test_restatement_against_the_reference_run_entries(fx, restated):
    assert len(fx["shims"]) >= 4
    for name in G.REFERENCE_PATH_CASES:
        key = ("hand/" if name in G.HAND_CASES else "skel/") + name
        nodes, edges, lengths, curves = restated[key][1][:4]
        assert np.array_equal(nodes[:, :2], fx["ref_nodes/" + name]), name
        assert len(curves) == 1 and np.array_equal(curves[0], fx["ref_curve/" + name]), name


def test_simplify_curve_against_the_reference_run_rdp(fx):
    from video.analysis import curves as C
    count = 0
    for name, curve in G.rdp_curves().items():
        assert np.array_equal(curve, fx["rdp_in/" + name]), name
        for eps in G.rdp_epsilons(curve):
            keep = curve.copy()
            got = C.simplify_curve(curve, eps)
            assert np.array_equal(curve, keep)
            want = fx["rdp/%s/%g" % (name, eps)]
            assert got.dtype == want.dtype and np.array_equal(got, want), (name, eps)
            count += 1
    assert count >= 4 * 3 + 4 * 2 and set(fx["rdp_ties"].tolist()) <= {"int%d/%g" % (k, e) for k in range(4)
                                                                       for e in G.RDP_EPSILONS}
    # float curves with epsilon 0 (the reference's rdp does not terminate there): every point that is off its chord stays
    for k in range(4):
        curve = fx["rdp_in/float%d" % k]
        assert np.array_equal(C.simplify_curve(curve, 0), curve)
    with pytest.raises(ValueError):
        C.simplify_curve(np.zeros((0, 2)), 0.1)


def test_merge_curves():
    from video.analysis import curves as C
    a, b = np.array([[0, 0], [1, 0], [2, 0]]), np.array([[2, 0], [2, 1]])
    want = [[0, 0], [1, 0], [2, 0], [2, 0], [2, 1]]
    assert C.merge_curves(a, b).tolist() == want
    assert C.merge_curves(a[::-1], b).tolist() == want
    assert C.merge_curves(a[::-1], b[::-1]).tolist() == want
    assert C.merge_curves(a, b[::-1]).tolist() == want
    with pytest.raises(ValueError):
        C.merge_curves(a, b + 5)


# ---------------------------------------------------------------------------------------- the graph class
def _graph(img, post_process=True):
    from video.analysis.morphological_graph import MorphologicalGraph
    nodes, edges, lengths, curves = G.skeleton_graph(img)
    return MorphologicalGraph.from_arrays(nodes, edges, curves, post_process), (nodes, edges, lengths, curves)


def test_import_video_does_not_need_networkx():
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import video, video.ops, video.analysis.shapes; "
            "assert 'networkx' not in sys.modules" % os.path.join(ROOT, "video-analysis_amd"))
    subprocess.check_call([sys.executable, "-c", code])


def test_graph_counts_and_insertion_order(restated):
    pytest.importorskip("networkx")
    from video.analysis import curves as C
    for name in ("hand/cross_x", "hand/ones5x9", "skel/blob2", "skel/ring3", "skel/comb7", "hand/nested2"):
        img = restated[name][0]
        g, (nodes, edges, lengths, curves) = _graph(img, post_process=False)
        assert list(g.nodes) == list(range(1, len(nodes) + 1)), name
        assert [g.nodes[k + 1]["coords"] for k in range(len(nodes))] == [tuple(n[:2]) for n in nodes.tolist()], name
        got = list(g.edges(keys=True, data=True))
        assert len(got) == len(edges) == g.number_of_edges(), name
        # between a pair of nodes, the edges keep the definition's order
        by_pair = {}
        for k in range(len(edges)):
            by_pair.setdefault(frozenset(edges[k, :2].tolist()), []).append(k)
        for pair, ks in by_pair.items():
            a, b = (min(pair) + 1, max(pair) + 1)
            datas = list(g.get_edge_data(a, b).values())
            assert len(datas) == len(ks), name
            for data, k in zip(datas, ks):
                assert np.array_equal(data["curve"], curves[k]) and data["length"] == lengths[k], name
                assert data["length"] == C.curve_length(data["curve"]), name
        assert [d for _, d in g.degree()] == nodes[:, 2].tolist(), name
        assert g.get_total_length() == sum(C.curve_length(c) for c in curves), name
        assert len(g.get_node_points()) == len(nodes) and len(g.get_edge_curves()) == len(edges), name


def test_graph_translate(restated):
    pytest.importorskip("networkx")
    g, (nodes, edges, lengths, curves) = _graph(restated["skel/blob0"][0], post_process=False)
    g.translate(7, -3)
    assert [g.nodes[k + 1]["coords"] for k in range(len(nodes))] == [(x + 7, y - 3) for x, y in nodes[:, :2].tolist()]
    got = sorted(c.tolist() for c in g.get_edge_curves())
    assert got == sorted((c + np.array([7, -3])).tolist() for c in curves)
    assert all(np.array_equal(c, k) for c, k in zip(curves, G.skeleton_graph(restated["skel/blob0"][0])[3]))


def test_post_processing_on_the_comb_and_ring_masks(restated):
    pytest.importorskip("networkx")
    # a comb of 4 teeth keeps its spine and teeth: 4 tips, 2 inner junctions (the outer teeth and the spine's ends
    # merge into one branch each), so 6 nodes become 4 tips + 2 junctions with 5 branches
    g, (nodes, edges, _, _) = _graph(restated["skel/comb4"][0])
    degrees = sorted(d for _, d in g.degree())
    assert degrees == [1, 1, 1, 1, 3, 3] and g.number_of_edges() == 5
    assert all(data["length"] >= 4 for _, _, data in g.edges(data=True))
    raw, _ = _graph(restated["skel/comb4"][0], post_process=False)
    assert g.get_total_length() <= raw.get_total_length()
    # a pure ring keeps its loop: one node of degree 2 whose only neighbour is itself
    for name in ("skel/ring1", "hand/ring4", "hand/diamond"):
        g, _ = _graph(restated[name][0])
        assert g.number_of_nodes() == 1 and g.number_of_edges() == 1, name
        (n1, n2, data), = g.edges(data=True)
        assert n1 == n2 and np.array_equal(data["curve"][0], data["curve"][-1]), name
    # a short spur at an end point goes, with its end point; simplify then merges the two edges left at the node
    spur = np.zeros((5, 12), np.uint8)
    spur[3, :] = 1
    spur[1:3, 6] = 1
    g, (nodes, edges, _, _) = _graph(spur)
    assert len(nodes) == 4 and len(edges) == 3
    assert g.number_of_nodes() == 2 and g.number_of_edges() == 1
    (n1, n2, data), = g.edges(data=True)
    assert sorted([g.nodes[n1]["coords"], g.nodes[n2]["coords"]]) == [(0, 3), (11, 3)]
    assert data["curve"].tolist() == [[x, 3] for x in range(7)] + [[x, 3] for x in range(6, 12)]
    # two sweeps: the second removes what the first one's removals turned into a short end branch
    g2, _ = _graph(spur, post_process=False)
    g2.remove_short_edges(20)
    assert g2.number_of_edges() == 0


def test_insert_node_and_closest_queries(restated):
    pytest.importorskip("networkx")
    g, (nodes, edges, lengths, curves) = _graph(restated["hand/row7"][0], post_process=False)
    node, coords, dist = g.get_closest_node((5, 1))
    assert (node, coords, dist) == (2, (6, 0), float(np.hypot(1, 1)))
    edge, point_id, dist = g.get_closest_edge((2.25, 2))
    assert edge == (1, 2, 0) and point_id == 2 and dist == float(np.hypot(0.25, 2))
    new = g.insert_node_into_edge((1, 2), 3)
    assert new == 3 and g.nodes[3]["coords"] == (3, 0)
    assert g.number_of_edges() == 2 and not g.has_edge(1, 2)
    assert g.get_single_edge_data(1, 3)["curve"].tolist() == [[x, 0] for x in range(4)]
    assert g.get_single_edge_data(3, 2)["curve"].tolist() == [[x, 0] for x in range(3, 7)]
    assert g.get_single_edge_data(1, 3)["length"] == 3.0 and g.get_point_on_edge(3, 2, 1).tolist() == [4, 0]
    assert g.add_node_point((3, 0)) == 3                                 # found, not added again
    g.add_and_connect_node_point((5, 4))
    assert g.number_of_nodes() == 5 and g.number_of_edges() == 4
    assert g.get_single_edge_data(4, 5)["curve"].tolist() == [[5, 4], [5, 0]]
    with pytest.raises(ValueError):
        g.add_edge_line(1, 2, [(0, 0), (1, 1)])
    g.simplify()                                                         # node 3 has degree 2 and goes again
    assert not g.has_node(3) and g.get_single_edge_data(1, 5)["curve"][-1].tolist() == [5, 0]
    # the point-to-segment distance picks the edge (every arm has the vertex (2, 2), the nearest one of each); the
    # distance returned is that to the nearest point of the edge's curve
    x, _ = _graph(restated["hand/cross_x"][0], post_process=False)
    x.edges[1, 3, 0]["curve"] = np.array([[0, 0], [2, 2]])
    edge, point_id, dist = x.get_closest_edge((1.2, 0.9))
    assert edge == (1, 3, 0) and point_id == 1 and dist == float(np.hypot(0.8, 1.1))
    empty, _ = _graph(np.zeros((3, 3), np.uint8))
    assert empty.get_closest_edge((0, 0)) == (None, None, np.inf) and empty.get_closest_node((0, 0))[0] is None
