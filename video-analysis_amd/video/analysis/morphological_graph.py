"""MorphologicalGraph: the graph of a skeleton image (reference: video/analysis/morphological_graph.py).

The reference walks the skeleton on the host and pops its seeds from a dict and a set, so its graphs depend on
the interpreter's hashing.  Here the nodes, edges and curves come from the GPU (ops.skeleton_graphs,
va_skeleton_graph) by the definition pinned in DESIGN.md §9, "Skeleton graphs", which depends on nothing but the
image; this module builds networkx graphs from those arrays and carries the reference's graph methods for
Python 3 and networkx 3.  networkx is imported here only, `import video` does not need it.

Post-processing (`remove_short_edges(4)`, then `simplify()`) follows the reference's rules with an iteration that
is defined here: a sweep of remove_short_edges works on a snapshot of the edge list in graph
order, skips edges that are gone by the time they are reached and takes the degrees when the edge is examined,
and sweeps repeat until one changes nothing; simplify restarts from the first node of degree 2 with two distinct
neighbours after each merge.  get_closest_edge measures point-to-segment distances with NumPy (no shapely).
"""
import networkx as nx
import numpy as np

from . import curves


def _segment_distance(point, curve):
    """the smallest distance from `point` to the segments of the (N, 2) curve (to its one point if N == 1)"""
    c = np.asarray(curve, np.float64).reshape(-1, 2)
    p = np.asarray(point, np.float64)
    if len(c) == 1:
        return float(np.hypot(*(c[0] - p)))
    a, d = c[:-1], c[1:] - c[:-1]
    dd = np.einsum("ij,ij->i", d, d)
    t = np.einsum("ij,ij->i", p - a, d) / np.where(dd > 0, dd, 1.0)
    foot = a + np.clip(np.where(dd > 0, t, 0.0), 0.0, 1.0)[:, None] * d
    return float(np.hypot(foot[:, 0] - p[0], foot[:, 1] - p[1]).min())


def _coincide(p, q):
    """True where two points are the same up to rounding"""
    return bool(np.allclose(p, q))


def _run_between(curve, start, end):
    """`curve` as an array that runs from `start` to `end`: itself, or reversed; ValueError if its end points are
    not those two"""
    curve = np.asarray(curve)
    if _coincide(curve[0], start) and _coincide(curve[-1], end):
        return curve
    if _coincide(curve[0], end) and _coincide(curve[-1], start):
        return curve[::-1]
    raise ValueError("the curve from %s to %s does not join the nodes at %s and %s"
                     % (tuple(curve[0]), tuple(curve[-1]), tuple(start), tuple(end)))


class MorphologicalGraph(nx.MultiGraph):
    """The graph of a skeleton: a networkx MultiGraph (two junctions may be joined by several branches, and a
    branch may return to its own junction).  A node carries `coords`, an (x, y) tuple.  An edge (n1, n2, key)
    carries `curve`, an (N, 2) array that runs from n1's coordinates to n2's, and `length`, its
    curves.curve_length."""

    def __init__(self, *args, **kwargs):
        super(MorphologicalGraph, self).__init__(*args, **kwargs)
        self._last_id = 0               # node ids handed out by add_node_point are _last_id + 1, + 2, ...

    # ------------------------------------------------------------------ reading
    def get_node_points(self):
        """the coordinates of every node, in node order"""
        return [coords for _, coords in self.nodes(data='coords')]

    def get_edge_curves(self):
        """the curve of every edge, in edge order"""
        return [curve for _, _, curve in self.edges(data='curve')]

    def get_single_edge_data(self, n1, n2):
        """the attributes of THE edge between n1 and n2; ValueError unless there is exactly one"""
        found = self.get_edge_data(n1, n2) or {}
        if len(found) != 1:
            raise ValueError("%d edges join the nodes %s and %s, exactly one is needed" % (len(found), n1, n2))
        (data,) = found.values()
        return data

    def get_point_on_edge(self, n1, n2, point_id):
        """point number `point_id` of the curve of the one edge between n1 and n2"""
        return self.get_single_edge_data(n1, n2)['curve'][point_id, :]

    def get_total_length(self):
        """the summed curve lengths of all edges, measured anew from the curves"""
        return sum(curves.curve_length(curve) for curve in self.get_edge_curves())

    def get_closest_node(self, point):
        """(node id, its coordinates, its distance) of the node nearest to `point`, the first one on ties;
        (None, None, inf) for a graph without nodes"""
        best = (None, None, np.inf)
        for node, coords in self.nodes(data='coords'):
            dist = curves.point_distance(point, coords)
            if dist < best[2]:
                best = (node, coords, dist)
        return best

    def get_closest_edge(self, point):
        """(edge, point id, distance): the edge (n1, n2, key) whose curve, taken as a chain of segments, passes
        nearest to `point` (the first one on ties), the index of the curve's point nearest to `point`, and the
        distance of that curve point.  (None, None, inf) for a graph without edges"""
        ranked = [(_segment_distance(point, curve), k) for k, (_, _, curve) in enumerate(self.edges(data='curve'))]
        if not ranked:
            return None, None, np.inf
        _, k = min(ranked)
        n1, n2, key, curve = list(self.edges(keys=True, data='curve'))[k]
        gaps = np.linalg.norm(np.asarray(curve, np.float64) - np.asarray(point, np.float64), axis=1)
        point_id = int(np.argmin(gaps))
        return (n1, n2, key), point_id, float(gaps[point_id])

    # ------------------------------------------------------------------ building
    def add_node_point(self, coords):
        """the id of the node at `coords`: an existing node that lies there, else a new one"""
        for node, have in self.nodes(data='coords'):
            if _coincide(coords, have):
                return node
        self._last_id += 1
        self.add_node(self._last_id, coords=coords)
        return self._last_id

    def add_edge_line(self, n1, n2, curve):
        """joins n1 and n2 by an edge along `curve`, which may be given in either direction and is stored running
        from n1 to n2.  A curve of no length (1e-6 or less) adds nothing.  ValueError if the curve does not join
        the two nodes"""
        curve = _run_between(curve, self.nodes[n1]['coords'], self.nodes[n2]['coords'])
        length = curves.curve_length(curve)
        if length > 1e-6:
            self.add_edge(n1, n2, curve=curve, length=length)

    def insert_node_into_edge(self, edge, point_id):
        """splits an edge at point `point_id` of its curve: a node at that point (a new one, or one that lies
        there already) takes over the two parts, and the edge itself goes.  `edge` is (n1, n2, key), or (n1, n2)
        for the first edge between the two.  Returns the node's id"""
        n1, n2 = edge[0], edge[1]
        key = edge[2] if len(edge) > 2 else next(iter(self[n1][n2]))
        curve = np.asarray(self.edges[n1, n2, key]['curve'])          # point_id counts along the curve as stored
        if _run_between(curve, self.nodes[n1]['coords'], self.nodes[n2]['coords']) is not curve:
            n1, n2 = n2, n1                                            # the stored curve starts at the other node
        middle = self.add_node_point(tuple(curve[point_id]))
        self.remove_edge(n1, n2, key)
        self.add_edge_line(n1, middle, curve[:point_id + 1])
        self.add_edge_line(middle, n2, curve[point_id:])
        return middle

    def connect_point_to_edge(self, point, edge, point_id):
        """a node at `point`, joined by a straight edge to a node inserted into `edge` at point `point_id` of its
        curve (`edge` as insert_node_into_edge takes it)"""
        outside = self.add_node_point(point)
        on_edge = self.insert_node_into_edge(edge, point_id)
        self.add_edge_line(outside, on_edge, [point, self.nodes[on_edge]['coords']])

    def add_and_connect_node_point(self, point):
        """a node at `point`, joined to the nearest edge at that edge's curve point nearest to it"""
        edge, point_id, _ = self.get_closest_edge(point)
        self.connect_point_to_edge(point, edge, point_id)

    # ------------------------------------------------------------------ changing
    def translate(self, x, y):
        """moves every node and every curve by (x, y)"""
        shift = np.array([x, y])
        for node in self.nodes:
            cx, cy = self.nodes[node]['coords']
            self.nodes[node]['coords'] = (cx + x, cy + y)
        for _, _, data in self.edges(data=True):
            data['curve'] = data['curve'] + shift

    def _sweep_short_edges(self, length_min, keep):
        """one sweep of remove_short_edges over a snapshot of the edge list; True if it removed anything"""
        removed = False
        for n1, n2, key, length in list(self.edges(keys=True, data='length')):
            if not self.has_edge(n1, n2, key) or length >= length_min or n1 in keep or n2 in keep:
                continue
            tips = [n for n in {n1, n2} if self.degree(n) == 1]     # degrees as they are now
            if tips:
                self.remove_nodes_from(tips)                        # the edge goes with its end point(s)
            elif n1 == n2:
                self.remove_edge(n1, n2, key)
            else:
                continue
            removed = True
        return removed

    def remove_short_edges(self, length_min=1, exclude_nodes=None):
        """prunes what is shorter than `length_min`: a branch that ends in an end point (a node of degree 1) goes
        together with that end point, and a loop goes; a short edge between two junctions stays.  Edges at a
        node of `exclude_nodes` are left alone.  Sweeps (see the module docstring) repeat until one removes
        nothing, since a removal can turn a junction into an end point"""
        keep = frozenset(exclude_nodes or ())
        while self._sweep_short_edges(length_min, keep):
            pass

    def _first_pass_through_node(self):
        """the first node, in node order, with exactly two edge ends that lead to two different nodes"""
        for node in self.nodes:
            if self.degree(node) == 2 and len(self[node]) == 2:
                return node
        return None

    def simplify(self, epsilon=0, simplify_curves=None):
        """removes every node that a curve merely passes through (degree 2, two distinct neighbours), merging its
        two edges into one, one node at a time from the front of the node list; a node with a loop, or with two
        edges to one neighbour, stays.  With epsilon > 0 every curve is then thinned by curves.simplify_curve and
        measured again.  simplify_curves: None, or a function (list of curves, epsilon) -> list of thinned curves
        that takes the place of the per-curve calls, e.g. curves.simplify_curves (one device call, the pinned
        form: see its docstring for where that differs from simplify_curve); the default path needs no GPU."""
        self.merge_pass_through_nodes()
        if epsilon > 0:
            self.set_curves(self.thinned_curves(epsilon, simplify_curves))

    def merge_pass_through_nodes(self):
        """the first step of simplify: the merges alone"""
        node = self._first_pass_through_node()
        while node is not None:
            left, right = self[node]
            merged = curves.merge_curves(self.get_single_edge_data(left, node)['curve'],
                                         self.get_single_edge_data(node, right)['curve'])
            self.remove_node(node)
            self.add_edge_line(left, right, merged)
            node = self._first_pass_through_node()

    def thinned_curves(self, epsilon, simplify_curves=None):
        """the curves of all edges, in edge order, thinned with epsilon"""
        given = [data['curve'] for _, _, data in self.edges(data=True)]
        if simplify_curves is None:
            return [curves.simplify_curve(c, epsilon) for c in given]
        return simplify_curves(given, epsilon)

    def set_curves(self, thinned):
        """the second step of simplify: every edge, in edge order, gets its thinned curve and is measured again"""
        for (_, _, data), curve in zip(self.edges(data=True), thinned):
            data['curve'] = curve
            data['length'] = curves.curve_length(curve)

    def post_process(self):
        """the clean-up from_skeleton applies by default: remove_short_edges(4), then simplify()"""
        self.remove_short_edges(4)
        self.simplify()

    @classmethod
    def from_arrays(cls, nodes, edges, curves_, post_process=True):
        """the graph of one item from the arrays of ops.skeleton_graphs (or of the definition's restatement); needs
        no GPU.  nodes: records or rows whose first fields are the anchor's x and y, in the definition's order --
        they become nodes 1 .. V; edges: records or rows with node_a, node_b (0-based) and, as records, `length`;
        curves_: one (N, 2) array per edge.  Edges are inserted in the given order."""
        graph = cls()
        named = getattr(nodes, "dtype", None) is not None and nodes.dtype.names
        for k in range(len(nodes)):
            x, y = (nodes["x"][k], nodes["y"][k]) if named else nodes[k][:2]
            graph.add_node(k + 1, coords=(int(x), int(y)))
        graph._last_id = len(nodes)
        named = getattr(edges, "dtype", None) is not None and edges.dtype.names
        for k in range(len(edges)):
            a, b = (edges["node_a"][k], edges["node_b"][k]) if named else edges[k][:2]
            curve = np.asarray(curves_[k])
            length = float(edges["length"][k]) if named else curves.curve_length(curve)
            graph.add_edge(int(a) + 1, int(b) + 1, curve=curve, length=length)
        if post_process:
            graph.post_process()
        return graph

    @classmethod
    def from_skeletons(cls, skeletons, post_process=True, stream=None):
        """the graphs of a list of 2-d skeleton images or of an (n, h, w) stack: one ops.skeleton_graphs call"""
        from .. import ops
        is_single = isinstance(skeletons, np.ndarray) and skeletons.ndim == 2
        res = ops.skeleton_graphs([skeletons] if is_single else skeletons, stream=stream)
        return [cls.from_arrays(g.nodes, g.edges, g.curves, post_process) for g in res]

    @classmethod
    def from_skeleton(cls, skeleton, copy=True, post_process=True):
        """the graph of one 2-d skeleton image (non-zero = foreground), from one ops.skeleton_graphs call.
        post_process: prune and merge as post_process() does.  `copy` is accepted for callers written against the
        reference's signature and has no effect: the image is never written to"""
        skeleton = np.asarray(skeleton)
        if skeleton.ndim != 2:
            raise ValueError("from_skeleton: expected a 2-d image, got shape %r" % (skeleton.shape,))
        return cls.from_skeletons([skeleton], post_process)[0]
