#!/usr/bin/env python3
"""Generates tests/golden/skeleton_graph_v1.npz -- skeleton graphs of masks by the pinned definition (DESIGN.md §9,
"Skeleton graphs"), and the two pieces of the reference that have an order-independent result.

    python tests/golden/make_golden_skeleton_graph.py <reference checkout>      (or set $VA_REFERENCE)

Importing this module needs no checkout: the tests take the restatement (`skeleton_graph`, pixel by pixel in the
definition's words), the hand cases with their expected nodes and curves, and the mask tables from it.  Writing
the fixture lifts, with `ast` at run time and in a namespace of shims, two pieces of the reference; none of their
source is stored, the fixture holds data only:

  rdp (external/simplify_polygon_rdp.py)                 with xrange -> range
  MorphologicalGraph.from_skeleton(post_process=False)   (video/analysis/morphological_graph.py) with
      cv2.filter2D -> a 3x3 neighbour count (zero beyond the border, saturated as uint8, which no case reaches);
      nx.MultiGraph -> a minimal base class with the networkx 1 calls the lifted code makes (add_node with a
      data dict, add_edge with attr_dict, .node); nx.get_node_attributes(...).iteritems -> a plain dict walk;
      curves.point_distance / curve_length -> the package's arithmetic restated here
  It runs only on skeletons that are single open paths (the four worm skeletons, the straight and the diagonal
  hand case): there its result depends on no dict or set order -- one seed, one walk, no branching.  Recorded:
  the node coordinates and the curve with repeated consecutive points dropped (the reference appends the start
  node's coordinates and then the start pixel itself).

rdp cases: in the float curves no two candidate distances of a splitting step tie within 1e-9 (asserted when the
fixture is written).  The integer curves, staircases of unit steps as skeleton curves are, do tie, exactly:
symmetric points have the same distance to the last bit in either implementation, and both take the first.
These cases are listed in the fixture's `rdp_ties` and kept, because simplify_curve agrees with the reference's
result on each (tests/test_skeleton_graph_host.py compares every one).  Float curves are not run with epsilon = 0:
the reference's rdp also measures the chord's own end point, np.linalg.det gives that point a distance of some
1e-17 instead of 0, which exceeds epsilon = 0, and the module then recurses on the same points without end.
Integer curves (exact zeros) run with every epsilon.
"""
import ast
import importlib.util
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "skeleton_graph_v1.npz")

# raster order of the 8 neighbours: (dx, dy)
DIRS = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))


def _sibling(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_THIN = None


def thinning():
    """make_golden_thinning, loaded on first use (its blobs need scipy)"""
    global _THIN
    if _THIN is None:
        _THIN = _sibling("make_golden_thinning")
    return _THIN


# ------------------------------------------------------------------------------------- restatement
def curve_length(points):
    """float32 sqrt(dx*dx + dy*dy) per segment, the roots added in double in point order"""
    total = 0.0
    for (x0, y0), (x1, y1) in zip(points[:-1], points[1:]):
        dx, dy = np.float32(x1) - np.float32(x0), np.float32(y1) - np.float32(y0)
        total += float(np.sqrt(np.float32(dx * dx) + np.float32(dy * dy), dtype=np.float32))
    return total


def skeleton_graph(img, detail=False):
    """the skeleton graph of one image by the pinned definition: (nodes, edges, curves) with
         nodes   (V, 4) int32   x, y of the anchor, graph degree (a loop counts twice), pixels of the set
         edges   (E, 3) int32   node_a, node_b (0-based numbers of the item), npoints
         lengths (E,) float64
         curves  list of E (npoints, 2) int32 arrays
       as the tuple (nodes, edges, lengths, curves); detail=True appends (node pixel sets, chain pixel lists)"""
    img = np.asarray(img)
    h, w = img.shape
    fg = [[bool(img[y, x] != 0) for x in range(w)] for y in range(h)]

    def is_fg(x, y):
        return 0 <= x < w and 0 <= y < h and fg[y][x]

    def adjacent(x, y):
        out = []
        for dx, dy in DIRS:
            if not is_fg(x + dx, y + dy):
                continue
            if dx != 0 and dy != 0 and (is_fg(x + dx, y) or is_fg(x, y + dy)):
                continue
            out.append((x + dx, y + dy))
        return out

    pixels = [(x, y) for y in range(h) for x in range(w) if fg[y][x]]
    adj = {p: adjacent(*p) for p in pixels}
    index = lambda p: p[1] * w + p[0]                                   # noqa: E731
    deg = {p: len(adj[p]) for p in pixels}
    assert all(d <= 4 for d in deg.values())

    # node pixels: d != 2, and the first pixel of every component that has none (a pure ring)
    node_px = {p for p in pixels if deg[p] != 2}
    seen = set()
    for p in pixels:                                                    # raster order: p is its component's first
        if p in seen:
            continue
        comp, todo = [], [p]
        seen.add(p)
        while todo:
            q = todo.pop()
            comp.append(q)
            for r in adj[q]:
                if r not in seen:
                    seen.add(r)
                    todo.append(r)
        if all(deg[q] == 2 for q in comp):
            node_px.add(p)

    # nodes: maximal adjacent sets of node pixels, numbered by their smallest index
    node_of, sets = {}, []
    for p in pixels:
        if p not in node_px or p in node_of:
            continue
        members, todo = [], [p]
        node_of[p] = len(sets)
        while todo:
            q = todo.pop()
            members.append(q)
            for r in adj[q]:
                if r in node_px and r not in node_of:
                    node_of[r] = len(sets)
                    todo.append(r)
        sets.append(sorted(members, key=index))
    anchors = [min(s, key=lambda q: (-deg[q], index(q))) for s in sets]

    # edges: one walk per edge end; the end with the smaller (index(a), index(c1)) owns the edge
    found, degree = [], [0] * len(sets)
    for a in pixels:
        if a not in node_px:
            continue
        for c1 in adj[a]:
            if c1 in node_px:
                continue
            degree[node_of[a]] += 1
            chain, prev, cur = [], a, c1
            while cur not in node_px:
                chain.append(cur)
                nxt = [q for q in adj[cur] if q != prev]
                assert len(nxt) == 1                                    # a chain pixel never has to choose
                prev, cur = cur, nxt[0]
            b, ck = cur, chain[-1]
            if (index(a), index(c1)) < (index(b), index(ck)):
                found.append(((index(a), index(c1)), a, b, chain))
    found.sort(key=lambda e: e[0])

    nodes = np.array([[anchors[k][0], anchors[k][1], degree[k], len(sets[k])] for k in range(len(sets))],
                     np.int32).reshape(-1, 4)
    edges, lengths, curves, chains = [], [], [], []
    for _, a, b, chain in found:
        na, nb = node_of[a], node_of[b]
        pts = [anchors[na]] + ([a] if a != anchors[na] else []) + chain + ([b] if b != anchors[nb] else []) + \
            [anchors[nb]]
        edges.append((na, nb, len(pts)))
        lengths.append(curve_length(pts))
        curves.append(np.array(pts, np.int32).reshape(-1, 2))
        chains.append(chain)
    out = (nodes, np.array(edges, np.int32).reshape(-1, 3), np.array(lengths, np.float64), curves)
    return out + (sets, chains) if detail else out


# ---------------------------------------------------------------------------------------- hand cases
def _img(rows):
    return np.array([[1 if c == "#" else 0 for c in r] for r in rows], np.uint8)


def square_ring(n, pad=0):
    m = np.zeros((n + 2 * pad, n + 2 * pad), np.uint8)
    m[pad:pad + n, pad:pad + n] = 1
    m[pad + 1:pad + n - 1, pad + 1:pad + n - 1] = 0
    return m


def nested_rings(count, gap=2):
    """`count` concentric square rings, `gap` pixels from one to the next"""
    n = 2 * gap * count
    m = np.zeros((n, n), np.uint8)
    for k in range(count):
        o = k * gap
        m[o:n - o, o:n - o] = 1
        m[o + 1:n - o - 1, o + 1:n - o - 1] = 0
    return m


def serpentine(h, w):
    """one 4-connected line that runs along every other row and turns at alternating ends"""
    m = np.zeros((h, w), np.uint8)
    m[::2, :] = 1
    for k, y in enumerate(range(1, h, 2)):
        m[y, w - 1 if k % 2 == 0 else 0] = 1
    return m


def _ring_curve(n, x0=0, y0=0):
    """the loop of an n x n square ring whose first pixel is (x0, y0): out along the top row (the smaller second
    index), down the right side, back along the bottom and up the left side"""
    top = [(x0 + i, y0) for i in range(n)]
    right = [(x0 + n - 1, y0 + i) for i in range(1, n)]
    bottom = [(x0 + i, y0 + n - 1) for i in range(n - 2, -1, -1)]
    left = [(x0, y0 + i) for i in range(n - 2, 0, -1)]
    return top + right + bottom + left + [(x0, y0)]


def _serpentine_curve(h, w):
    pts = []
    for k, y in enumerate(range(0, h, 2)):
        row = [(x, y) for x in range(w)]
        pts += row if k % 2 == 0 else row[::-1]
        if y + 1 < h:
            pts.append((w - 1 if k % 2 == 0 else 0, y + 1))
    return pts


R2 = float(np.sqrt(np.float32(2), dtype=np.float32))

# name -> (mask, nodes [(x, y, degree, pixels)], edges [(node_a, node_b, [points])]), worked by hand
HAND_CASES = {
    "dot": (_img(["...", ".#.", "..."]), [(1, 1, 0, 1)], []),
    "pair": (_img(["##"]), [(0, 0, 0, 2)], []),
    "row3": (_img(["###"]), [(0, 0, 1, 1), (2, 0, 1, 1)], [(0, 1, [(0, 0), (1, 0), (2, 0)])]),
    "row7": (_img(["#######"]), [(0, 0, 1, 1), (6, 0, 1, 1)], [(0, 1, [(x, 0) for x in range(7)])]),
    "diag3": (_img(["#..", ".#.", "..#"]), [(0, 0, 1, 1), (2, 2, 1, 1)], [(0, 1, [(0, 0), (1, 1), (2, 2)])]),
    "diag6": (_img(["#.....", ".#....", "..#...", "...#..", "....#.", ".....#"]),
              [(0, 0, 1, 1), (5, 5, 1, 1)], [(0, 1, [(k, k) for k in range(6)])]),
    # the corner pixel (2, 0) has N/E/S/W neighbours (1, 0) and (2, 1) only; (1, 0) and (2, 1) touch at a corner
    # but share the foreground pixel (2, 0), so they are not adjacent: one plain edge
    "corner_l": (_img(["###", "..#", "..#"]), [(0, 0, 1, 1), (2, 2, 1, 1)],
                 [(0, 1, [(0, 0), (1, 0), (2, 0), (2, 1), (2, 2)])]),
    "cross_t": (_img(["#####", "..#..", "..#.."]), [(0, 0, 1, 1), (2, 0, 3, 1), (4, 0, 1, 1), (2, 2, 1, 1)],
                [(0, 1, [(0, 0), (1, 0), (2, 0)]), (1, 2, [(2, 0), (3, 0), (4, 0)]),
                 (1, 3, [(2, 0), (2, 1), (2, 2)])]),
    "cross_x": (_img(["#...#", ".#.#.", "..#..", ".#.#.", "#...#"]),
                [(0, 0, 1, 1), (4, 0, 1, 1), (2, 2, 4, 1), (0, 4, 1, 1), (4, 4, 1, 1)],
                [(0, 2, [(0, 0), (1, 1), (2, 2)]), (1, 2, [(4, 0), (3, 1), (2, 2)]),
                 (2, 3, [(2, 2), (1, 3), (0, 4)]), (2, 4, [(2, 2), (3, 3), (4, 4)])]),
    "cross_y": (_img(["#...#", ".#.#.", "..#..", "..#..", "..#.."]),
                [(0, 0, 1, 1), (4, 0, 1, 1), (2, 2, 3, 1), (2, 4, 1, 1)],
                [(0, 2, [(0, 0), (1, 1), (2, 2)]), (1, 2, [(4, 0), (3, 1), (2, 2)]),
                 (2, 3, [(2, 2), (2, 3), (2, 4)])]),
    "diamond": (_img([".#.", "#.#", ".#."]), [(1, 0, 2, 1)], [(0, 0, [(1, 0), (0, 1), (1, 2), (2, 1), (1, 0)])]),
    "ring4": (square_ring(4), [(0, 0, 2, 1)], [(0, 0, _ring_curve(4))]),
    "nested2": (nested_rings(2), [(0, 0, 2, 1), (2, 2, 2, 1)],
                [(0, 0, _ring_curve(8)), (1, 1, _ring_curve(4, 2, 2))]),
    "serpentine": (serpentine(15, 16), [(0, 0, 1, 1), (0, 14, 1, 1)], [(0, 1, _serpentine_curve(15, 16))]),
    # every pixel of a 2 x 2 block has its two edge neighbours (the diagonal shares foreground): a pure ring
    "ones2x2": (np.ones((2, 2), np.uint8), [(0, 0, 2, 1)], [(0, 0, [(0, 0), (1, 0), (1, 1), (0, 1), (0, 0)])]),
    # corners have d = 2 and are chain pixels: four loops of one chain pixel at the one node of 41 pixels, whose
    # anchor is its first pixel of d = 4, (1, 1)
    "ones5x9": (np.ones((5, 9), np.uint8), [(1, 1, 8, 41)],
                [(0, 0, [(1, 1), (1, 0), (0, 0), (0, 1), (1, 1)]),
                 (0, 0, [(1, 1), (7, 0), (8, 0), (8, 1), (1, 1)]),
                 (0, 0, [(1, 1), (0, 3), (0, 4), (1, 4), (1, 1)]),
                 (0, 0, [(1, 1), (8, 3), (8, 4), (7, 4), (1, 1)])]),
}
# single open paths: the reference's own from_skeleton is order-independent on these
REFERENCE_PATH_CASES = ("row3", "row7", "diag3", "diag6", "worm0", "worm1", "worm2", "worm3")


def fixture_skeletons():
    """name -> Guo-Hall skeleton of every mask of make_golden_thinning.fixture_masks()"""
    T = thinning()
    return {name: T.guo_hall(mask)[0] for name, mask in T.fixture_masks().items()}


def all_cases():
    """name -> image of every case of the fixture: the hand cases, then the thinning fixture's skeletons"""
    cases = {"hand/" + name: c[0] for name, c in HAND_CASES.items()}
    cases.update(("skel/" + name, s) for name, s in fixture_skeletons().items())
    return cases


def border_items():
    """items of every width 1 .. 70 with foreground in column 0 and w - 1 and in the first and last row; packed
    one after the other, a neighbourhood that reads across an item's border meets the next item's pixels"""
    rng = np.random.default_rng(11)
    out = []
    for w in range(1, 71):
        h = 1 + (w * 7) % 6
        m = (rng.random((h, w)) < 0.35).astype(np.uint8)
        m[:, 0] = m[:, -1] = 1
        m[0, ::2] = m[-1, 1::2] = 1
        if w % 3 == 0:
            m[0, :] = 1
        out.append(("border_w%d_h%d" % (w, h), m))
    return out


RDP_EPSILONS = (0.0, 0.1, 1.5)


def rdp_epsilons(curve):
    """the epsilons a curve is run with (the module docstring says why float curves skip 0)"""
    return RDP_EPSILONS if np.issubdtype(np.asarray(curve).dtype, np.integer) else RDP_EPSILONS[1:]


def rdp_curves():
    """name -> (N, 2) curve for simplify_curve: integer skeleton-like curves and float curves"""
    rng = np.random.default_rng(5)
    out = {}
    steps = np.array([(1, 0), (1, 1), (0, 1), (1, -1)])
    for k in range(4):
        out["int%d" % k] = np.cumsum(steps[rng.integers(0, 4, 40 + 17 * k)], axis=0).astype(np.int64)
    for k in range(4):
        t = np.linspace(0, 3 + k, 30 + 11 * k)
        out["float%d" % k] = np.c_[20 * t + rng.normal(0, 0.7, t.size), 9 * np.sin(t * 1.3) + rng.normal(0, 0.7, t.size)]
    out["two"] = np.array([[0.0, 0.0], [3.0, 4.0]])
    out["two_int"] = np.array([[0, 0], [3, 4]])
    out["vertical"] = np.array([[2.0, 0.0], [2.5, 1.0], [2.0, 2.0], [1.0, 3.5], [2.0, 5.0]])
    return out


# -------------------------------------------------------------------------------------------- lifting
def _lift(path, names, ns, rewrite=None):
    """exec the named top-level functions / classes of a reference file in the namespace `ns`"""
    src = open(path).read()
    if rewrite:
        src = rewrite(src)
    tree = ast.parse(src)
    body = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    assert len(body) == len(names), (path, names)
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)


def load_reference(root):
    """(rdp, from_skeleton) of the reference, lifted"""
    ns = {"np": np, "xrange": range}
    _lift(os.path.join(root, "external", "simplify_polygon_rdp.py"), ("pldist", "_rdp", "_rdp_nn", "rdp"), ns)
    ns["_rdp"].__defaults__ = None
    rdp = ns["rdp"]

    class Base(object):                              # the networkx 1 calls from_skeleton(post_process=False) makes
        def __init__(self):
            self.node, self.edge_list = {}, []

        def add_node(self, n, data):
            self.node[n] = dict(data)

        def add_edge(self, n1, n2, attr_dict):
            self.edge_list.append((n1, n2, dict(attr_dict)))

    class _Attrs(dict):
        def iteritems(self):
            return iter(self.items())

    class nx(object):
        MultiGraph = Base

        @staticmethod
        def get_node_attributes(g, name):
            return _Attrs((k, v[name]) for k, v in g.node.items())

    class curves(object):
        point_distance = staticmethod(lambda p1, p2: float(np.hypot(p1[0] - p2[0], p1[1] - p2[1])))
        curve_length = staticmethod(lambda pts: curve_length([tuple(p) for p in np.asarray(pts)]))

    class cv2(object):
        @staticmethod
        def filter2D(img, ddepth, kernel):
            assert ddepth == -1 and kernel.shape == (3, 3) and kernel[1, 1] == 0 and kernel.sum() == 8
            p = np.pad(img.astype(np.int64), 1)
            h, w = img.shape
            s = sum(p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dx, dy in DIRS)
            return np.minimum(s, 255).astype(img.dtype)

    ns2 = {"np": np, "nx": nx, "cv2": cv2, "curves": curves, "__name__": "ref_graph"}

    def py3(src):                                    # the module is Python 2: print statements become `pass`
        return re.sub(r"(?m)^(\s*)print\s+[^(\n][^\n]*$", r"\1pass", src)
    _lift(os.path.join(root, "video", "analysis", "morphological_graph.py"), ("MorphologicalGraph",), ns2, py3)

    def from_skeleton(skel):
        g = ns2["MorphologicalGraph"].from_skeleton(np.pad((np.asarray(skel) != 0).astype(np.uint8), 1),
                                                    copy=True, post_process=False)
        nodes = np.array([g.node[k]["coords"] for k in sorted(g.node)], np.int64).reshape(-1, 2) - 1
        curves_ = []
        for n1, n2, data in g.edge_list:
            c = np.asarray(data["curve"], np.int64).reshape(-1, 2) - 1
            keep = np.r_[True, np.any(c[1:] != c[:-1], axis=1)]
            curves_.append(c[keep])
        return nodes, curves_
    return rdp, from_skeleton


def _rdp_ties(M, eps, pldist):
    """True if, at some step of the recursion that splits, the two largest candidate distances lie within 1e-9"""
    if len(M) <= 2:
        return False
    d = np.array([float(pldist(M[i], M[0], M[-1])) for i in range(1, len(M) - 1)])
    if d.max() <= eps:
        return False
    top = np.sort(d)[::-1]
    i = 1 + int(np.argmax(d))
    return (len(top) > 1 and top[0] - top[1] <= 1e-9) or _rdp_ties(M[:i + 1], eps, pldist) or \
        _rdp_ties(M[i:], eps, pldist)


def generate(root):
    rdp, from_skeleton = load_reference(root)
    data = {"shims": np.array(["xrange -> range", "cv2.filter2D -> 3x3 neighbour count, zero border",
                               "nx.MultiGraph -> add_node / add_edge(attr_dict) / .node",
                               "curves.point_distance, curve_length -> restated"])}
    for name, img in all_cases().items():
        nodes, edges, lengths, curves_ = skeleton_graph(img)
        data["img/" + name] = img
        data["nodes/" + name] = nodes
        data["edges/" + name] = edges
        data["lengths/" + name] = lengths
        data["points/" + name] = np.concatenate(curves_ + [np.zeros((0, 2), np.int32)]).astype(np.int32)
    for name in REFERENCE_PATH_CASES:
        img = all_cases()[("hand/" if name in HAND_CASES else "skel/") + name]
        nodes, curves_ = from_skeleton(img)
        assert len(curves_) == 1, name
        data["ref_nodes/" + name] = nodes
        data["ref_curve/" + name] = curves_[0]
    pldist = rdp.__globals__["pldist"]
    ties = []
    for name, curve in rdp_curves().items():
        data["rdp_in/" + name] = curve
        for eps in rdp_epsilons(curve):
            if _rdp_ties(curve, eps, pldist):
                assert np.issubdtype(curve.dtype, np.integer), (name, eps)
                ties.append("%s/%g" % (name, eps))
            data["rdp/%s/%g" % (name, eps)] = np.asarray(rdp(curve.copy(), eps))
    data["rdp_ties"] = np.array(ties)
    return data


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("VA_REFERENCE")
    if not root or not os.path.isdir(os.path.join(root, "video", "analysis")):
        sys.stderr.write("usage: make_golden_skeleton_graph.py <reference checkout> (or $VA_REFERENCE); nothing "
                         "written\n")
        raise SystemExit(2)
    data = generate(root)
    np.savez_compressed(OUT, **data)
    print("wrote %s (%d arrays, %d bytes)" % (OUT, len(data), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
