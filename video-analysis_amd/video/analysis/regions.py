"""Region helpers: rectangles (host arithmetic) and blob detection (GPU).

Reference: video/analysis/regions.py -- corners_to_rect :23-29, rect_to_corners :33-45,
rect_to_slices :49-53, get_overlapping_slices :57-110, find_bounding_box :113-149,
expand_rectangle :153-155, get_largest_region :159-174, triangle_area :430-451,
make_distance_map :455-509, shortest_path_in_distance_map :513-565, get_farthest_points :568-611,
get_external_contour :201-232 (and every cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) list: find_contours),
get_ray_hitpoint :353-391, get_ray_intersections :395-405, get_farthest_ray_intersection :409-426 (GPU; batched:
ray_hits, ray_fans), simplify_contour :307-325 (GPU; batched: simplify_contours).
"""
import numpy as np


def corners_to_rect(p1, p2):
    """rectangle (left, top, width, height) spanned by two corner points, both included"""
    xmin, xmax = min(p1[0], p2[0]), max(p1[0], p2[0])
    ymin, ymax = min(p1[1], p2[1]), max(p1[1], p2[1])
    return (xmin, ymin, xmax - xmin + 1, ymax - ymin + 1)


def rect_to_corners(rect, count=2):
    """`count` (2 or 4) corner points of a rectangle; the points lie inside it"""
    p1 = (rect[0], rect[1])
    p2 = (rect[0] + rect[2] - 1, rect[1] + rect[3] - 1)
    if count == 2:
        return p1, p2
    if count == 4:
        return p1, (p2[0], p1[1]), p2, (p1[0], p2[1])
    raise ValueError("count must be 2 or 4 (cannot be %d)" % count)


def rect_to_slices(rect):
    """(slice_y, slice_x) selecting the rectangle from an array"""
    return slice(rect[1], rect[1] + rect[3]), slice(rect[0], rect[0] + rect[2])


def get_overlapping_slices(t_pos, t_shape, i_shape, anchor='center', ret_rect=False):
    """slices that cut the common part out of a template placed in a larger image
    (reference :57-110).  t_pos = (x, y) of the template's anchor in the image, t_shape =
    (height, width) of the template, i_shape = (height, width) of the image.  Returns
    ((template_rows, template_cols), (image_rows, image_cols)) and, with ret_rect, the common
    rectangle (left, top, width, height) in image coordinates; RuntimeError if nothing overlaps."""
    th, tw = t_shape[0], t_shape[1]
    if anchor == 'center':
        left, top = t_pos[0] - tw // 2, t_pos[1] - th // 2
    elif anchor == 'upper left':
        left, top = t_pos[0], t_pos[1]
    else:
        raise ValueError('Unknown anchor point: %s' % anchor)

    def overlap(start, t_len, i_len):
        """(image start, template start, length) along one axis"""
        length = min(t_len, i_len - start)
        if length <= 0 or start <= -t_len:
            raise RuntimeError('Template and image do not overlap')
        if start >= 0:
            return start, 0, length
        return 0, -start, length + start

    i_x, t_x, w = overlap(left, tw, i_shape[1])
    i_y, t_y, h = overlap(top, th, i_shape[0])
    slices = ((slice(t_y, t_y + h), slice(t_x, t_x + w)),
              (slice(i_y, i_y + h), slice(i_x, i_x + w)))
    if ret_rect:
        return slices, (i_x, i_y, w, h)
    return slices


def triangle_area(a, b, c):
    """area of a triangle with side lengths a, b, c (numbers or arrays) by Heron's formula;
    radicands that rounding made negative give 0 (reference :430-451)"""
    s = (a + b + c) / 2
    radicand = s * (s - a) * (s - b) * (s - c)
    if isinstance(radicand, np.ndarray):
        return np.sqrt(np.where(radicand > 0, radicand, 0))
    return np.sqrt(radicand) if radicand > 0 else 0


def expand_rectangle(rect, amount=1):
    return (rect[0] - amount, rect[1] - amount, rect[2] + 2 * amount, rect[3] + 2 * amount)


def label(mask, connectivity=4):
    """(labels, num_features) like scipy.ndimage.label -- the call get_largest_region makes
    at regions.py:162 -- computed by the run-based union-find kernels on the GPU"""
    from .. import ops
    return ops.label(mask, connectivity)


def find_bounding_box(mask):
    """(left, top, width, height) of the white region of a mask, the reference's result for every
    mask: top / left are the first occupied row / column, and the box ends at the first EMPTY row /
    column after them (or at the edge).  For a region whose occupied rows and columns are each
    contiguous -- every connected region -- this is the bounding box; otherwise it stops at the
    first gap.  The bounding box comes from the GPU's region statistics; the row and column
    occupancy inside it is a host reduction.  An empty mask raises IndexError."""
    from .. import ops
    m = np.asarray(mask) != 0
    st = ops.region_stats(m.astype(np.int32), 1)[0]
    if st[0] == 0:
        raise IndexError("mask is empty")
    xmin, ymin, xmax, ymax = (int(v) for v in st[10:14])
    box = m[ymin:ymax + 1, xmin:xmax + 1]

    def run(occupied):
        """length of the leading run of occupied rows / columns (the first one is occupied)"""
        gaps = np.flatnonzero(~occupied)
        return int(gaps[0]) if len(gaps) else len(occupied)
    return (xmin, ymin, run(box.any(axis=0)), run(box.any(axis=1)))


def get_largest_region(mask, ret_area=False, connectivity=4):
    """boolean mask that only contains the largest 4-connected region (first one on ties);
    ValueError on an empty mask, like np.argmax([]) in the reference"""
    from .. import ops
    region, area, count = ops.largest_region(mask, connectivity)
    if count == 0:
        raise ValueError("attempt to get argmax of an empty sequence")
    if ret_area:
        return region, area
    return region


def get_contour_from_largest_region(mask, ret_area=False):
    """contour of the region with the largest contour area as an (N, 2) float64 array of (x, y)
    points -- cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) + cv2.contourArea + argmax,
    reference: video/analysis/regions.py:178-197.  RuntimeError when the mask is empty."""
    from .. import ops
    points, area, count = ops.largest_contour(mask)
    if count == 0:
        raise RuntimeError("Could not find any contour")
    contour = np.squeeze(np.asarray(points.reshape(-1, 1, 2), np.double))
    if ret_area:
        return contour, area
    return contour


def find_contours(mask):
    """cv2.findContours(mask.astype(np.uint8), cv2.RETR_EXTERNAL, cv2.CHAIN_APPROX_SIMPLE)[1]: the list of
    (N, 1, 2) int32 outer contours in OpenCV's order (reference: video/analysis/regions.py:180-182, :229-231,
    :575-576; video/io/composer.py:228).  A stack (n, h, w) gives one list per frame, from one call."""
    from .. import ops
    return ops.find_contours(mask)


def _contour_points(contour, closed, what):
    """the (n, 2) points of one contour: an (n, 2) array-like or an (n, 1, 2) array as find_contours gives; a ring's
    closing duplicate is dropped.  A shapely geometry is a TypeError"""
    if any(hasattr(contour, name) for name in ("coords", "exterior", "geom_type")):
        raise TypeError("%s takes the coordinates of a contour as an (n, 2) array, not a %s: pass "
                        "np.asarray(geometry.coords) (for a polygon, of its exterior)" % (what, type(contour).__name__))
    a = np.asarray(contour)
    if a.ndim == 3 and a.shape[1] == 1:
        a = a[:, 0, :]
    if a.size == 0:
        a = a.reshape(0, 2)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("%s: a contour is an (n, 2) array, got shape %r" % (what, a.shape))
    if closed and len(a) >= 2 and a[0, 0] == a[-1, 0] and a[0, 1] == a[-1, 1]:
        a = a[:-1]
    return a


def _is_frame_list(entry):
    """whether an entry of simplify_contours' argument is one frame's list of contours, as find_contours returns
    for a stack, and not a contour"""
    return isinstance(entry, (list, tuple)) and all(isinstance(c, np.ndarray) and c.ndim >= 2 for c in entry)


def simplify_contours(contours, threshold, closed=True):
    """simplify_contour for every contour of a list in one device call (ops.simplify_curves, Visvalingam, DESIGN.md
    §9, "Simplification").  contours: what find_contours returns, as it is -- a list of (N, 1, 2) contours, or for a
    stack one such list per frame -- or any list of (n, 2) array-likes.  threshold: one number or one per contour
    (for a stack: one number).  closed=True takes each contour as a ring, a closing duplicate point dropped first;
    closed=False as an open line whose ends stay.  Returns, in the layout of the argument, the kept (K, 2) points
    of every contour in its dtype; None for a ring that vanishes (fewer than 3 points are left, or were given)."""
    from .. import ops
    what = "simplify_contours"
    contours = list(contours)
    if contours and all(_is_frame_list(entry) for entry in contours):
        if np.ndim(threshold) != 0:
            raise ValueError("%s: one threshold for the contours of a stack" % what)
        flat = simplify_contours([c for frame in contours for c in frame], threshold, closed)
        out, at = [], 0
        for frame in contours:
            out.append(flat[at:at + len(frame)])
            at += len(frame)
        return out
    rings = [_contour_points(c, closed, what) for c in contours]
    return ops.simplify_curves(rings, threshold, method="visvalingam", closed=closed)


def simplify_contour(contour, threshold):
    """simplifies a contour based on its area: single points are removed while the area change of the resulting
    polygon is smaller than `threshold` (Visvalingam; reference: video/analysis/regions.py:307-325 over
    external/simplify_polygon_visvalingam.py).  contour: the coordinates of a linear ring, an (n, 2) array-like; a
    closing duplicate point is dropped first.  Returns the kept points, a (K, 2) array of the input's dtype, or None
    when fewer than 3 would be left.  Deviations: the reference returns the coordinates of a shapely ring, which
    shapely has closed again and the reference then cut by one point, so a result whose last kept point equals its
    first loses that point there and keeps it here; the shapely forms of the argument (LineString, LinearRing,
    Polygon) are a TypeError that names the array form.  Fewer than 3 points are a ValueError, as they are for
    shapely's LinearRing."""
    ring = _contour_points(contour, True, "simplify_contour")
    if len(ring) < 3:
        raise ValueError("simplify_contour: a linear ring needs at least 3 points, got %d" % len(ring))
    return simplify_contours([ring], threshold)[0]


def external_contour_resolution(points):
    """get_external_contour's default resolution: half the smallest non-zero distance of consecutive points, the
    closing pair included, but at least a 2048th of the ring's longest side (reference :204-215)"""
    p = np.asarray(points, np.double).reshape(-1, 2)
    dist = np.hypot(*(p - np.roll(p, 1, axis=0)).T)
    if not np.any(dist > 0):
        raise ValueError("the points of the ring coincide: no resolution follows from them")
    return max(0.5 * dist[dist > 0].min(), np.ptp(p, axis=0).max() / 2048)


def get_external_contours(list_of_points, resolution=None):
    """get_external_contour for every ring of a list: one fill launch and one contour launch for all of them.
    resolution: None (each ring's own default), one number, or one per ring.  Every ring is filled into a box of
    one common size (its own origin, zero padding to the right and below, which changes no contour), so that the
    masks form a uniform stack.  Returns the list of (N, 2) float64 contours."""
    from .. import ops
    rings = [np.asarray(p, np.double).reshape(-1, 2) for p in list_of_points]
    m = len(rings)
    if m == 0:
        return []
    if resolution is None or np.ndim(resolution) == 0:
        resolution = [resolution] * m
    if len(resolution) != m:
        raise ValueError("need one resolution per ring (%d rings, %d resolutions)" % (m, len(resolution)))
    res = [external_contour_resolution(p) if r is None else float(r) for p, r in zip(rings, resolution)]
    ints = [np.array(p / r, np.int64) for p, r in zip(rings, res)]         # truncation towards zero, as np.int
    origin = np.array([c.min(axis=0) - 1 for c in ints])
    size = np.max([np.ptp(c, axis=0) + 3 for c in ints], axis=0)
    boxes = np.concatenate([origin, np.broadcast_to(size, (m, 2))], axis=1)
    masks = np.stack(ops.fill_polys(ints, boxes))
    out = []
    for k, contours in enumerate(ops.find_contours(masks)):
        if len(contours) != 1:
            raise RuntimeError("ring %d filled into %d components" % (k, len(contours)))
        out.append((contours[0].reshape(-1, 2) + origin[k]) * res[k])
    return out


def get_external_contour(points, resolution=None):
    """approximation of the external contour of a linear ring `points`, which may intersect itself: the ring is
    scaled to integers by `resolution` (default: external_contour_resolution), filled (cv2.fillPoly) into a mask
    one pixel larger on every side, and the mask's outer contour scaled back; reference:
    video/analysis/regions.py:201-232.  Returns an (N, 2) float64 array.  Deviation: a contour of one point is
    (1, 2), where the reference's np.squeeze gives (2,).  More than ops.FILL_MAX_VERTS points raise the fill's
    ValueError."""
    return get_external_contours([points], resolution)[0]


def make_distance_map(mask, start_points, end_points=None):
    """fills the pixels equal to 1 of the integer array `mask` (int32 or int64, changed in place)
    with 2 + the 8-neighbour geodesic distance to the nearest start point (x, y), as int(2 + d);
    reference: video/analysis/regions.py:455-509.  Other values are walls and stay as they are, as
    do pixels equal to 1 that cannot be reached; start points outside the array or on a pixel that
    is not 1 are ignored.  With end_points the fill stops at the nearest reachable one: the pixels
    closer than it are filled, and it itself.  Deviation: other pixels at exactly its distance stay
    unfilled (the reference's choice among them follows its float keys and set order).  Returns None."""
    from .. import ops
    if not isinstance(mask, np.ndarray) or mask.dtype not in (np.int32, np.int64):
        raise TypeError("make_distance_map works in place on an int32 or int64 array")
    if mask.ndim != 2:
        raise ValueError("mask must be 2-d")
    out = ops.distance_map(mask == 1, list(start_points),
                           None if end_points is None else list(end_points))
    filled = out >= 2
    mask[filled] = out[filled]


def shortest_path_in_distance_map(distance_map, end_point):
    """(N, 2) int64 array of the (x, y) points walked from `end_point` down the distance map to a
    minimum; reference: video/analysis/regions.py:513-565, step for step.  Deviation: an end point
    whose value is <= 1 (or that lies outside the map) raises ValueError, where the reference walks
    through its sentinels."""
    from .. import ops
    path = ops.distance_map_path(np.asarray(distance_map), end_point)
    if len(path) == 0:
        raise ValueError("end point %s is not a filled pixel of the distance map" % (tuple(end_point),))
    return path


def get_farthest_points(mask, p1=None, ret_path=False):
    """the two points of the mask's foreground (non-zero) farthest apart along geodesics, found by
    repeating distance maps from the farthest point of the last one; reference:
    video/analysis/regions.py:568-611.  p1 defaults to the first point of the longest external
    contour (cv2.arcLength).  Returns (p1, p2) as tuples of ints, or with ret_path the path from p2
    as shortest_path_in_distance_map gives it.  A p1 outside the frame or off the mask is ignored by
    the first map, as in the reference, so p2 moves to the first foreground pixel.  ValueError for an
    empty mask without p1 (max() of no contours in the reference), and for ret_path when no pixel
    was reached.  Deviation: every non-zero pixel is foreground.  The reference's np.clip(mask, 0, 1)
    agrees for bool and unsigned masks, but in signed masks it makes negative values background."""
    from .. import ops
    m = np.asarray(mask)
    if m.ndim != 2:
        raise ValueError("mask must be 2-d")
    if ret_path:
        path = ops.farthest_points(m, p1, ret_path=True)
        if len(path) == 0:
            raise ValueError("max() arg is an empty sequence" if p1 is None else "no pixel of the mask was reached")
        return path
    a, b, _, rounds = ops.farthest_points(m, p1, ret_stats=True)
    if p1 is None and a[0] == -1 and a[1] == -1:
        raise ValueError("max() arg is an empty sequence")
    if p1 is not None and rounds[0] == 1:     # never replaced: the caller's own start, as given
        return (int(p1[0]), int(p1[1])), (int(b[0]), int(b[1]))
    return (int(a[0]), int(a[1])), (int(b[0]), int(b[1]))


# ------------------------------------------------------------------------------------------ rays onto outlines
def _outline(shape):
    """(points (n, 2) float64, closed) of an outline argument ("Outline queries"): one of our Polygons
    is its contour, closed; an object with .coords is np.asarray(obj.coords), as given; anything else is an (N, 2)
    array-like, an open line string as given"""
    from .shapes import Polygon
    if isinstance(shape, Polygon):
        return shape.contour, True
    if hasattr(shape, "coords"):
        shape = shape.coords
    pts = np.asarray(shape, np.float64)
    return (pts.reshape(0, 2) if pts.size == 0 else pts), False


def _hit_distances(hits, anchors):
    """the pinned distance sqrt(dx dx + dy dy) of hit points from their anchors (NaN rows stay NaN)"""
    with np.errstate(all="ignore"):
        dx, dy = hits[:, 0] - anchors[:, 0], hits[:, 1] - anchors[:, 1]
        return np.sqrt(dx * dx + dy * dy)


def _far_points(anchor, angles, ray_length):
    """the reference's far point of every angle, evaluated angle by angle as its loop does (:401-402)"""
    return [(anchor[0] + ray_length * np.cos(angle), anchor[1] + ray_length * np.sin(angle)) for angle in angles]


def ray_hits(outlines, anchors, fars, index=None):
    """get_ray_hitpoint for q rays onto many outlines in one launch.  outlines: a list of outline arguments (see
    get_ray_hitpoint); anchors, fars: (q, 2); index: the outline of each ray (None: the one outline for all rays,
    else ray k onto outline k, which needs as many rays as outlines).  Returns (hits (q, 2) float64 with NaN rows
    for the rays that hit nothing, distances (q,) float64, NaN likewise, edges (q,) int32, -1 likewise)."""
    from .. import ops
    pts, closed = zip(*[_outline(o) for o in outlines]) if len(outlines) else ((), ())
    a = np.asarray(anchors, np.float64).reshape(-1, 2)
    _, hits, edge, _ = ops.ray_hits(list(pts), list(closed), a, fars, index)
    return hits, _hit_distances(hits, a), edge


def ray_fans(outlines, anchors, angles, ray_length=1000):
    """get_ray_intersections for many outlines in one launch: outline k gets the rays from anchors[k] at
    angles[k] (a list of angles per outline, of any lengths).  Returns one (hits (k, 2), distances (k,)) pair per
    outline, NaN where a ray hits nothing."""
    if not len(outlines) == len(anchors) == len(angles):
        raise ValueError("ray_fans: %d outlines, %d anchors and %d angle lists" % (len(outlines), len(anchors),
                                                                                  len(angles)))
    fars = [far for anchor, fan in zip(anchors, angles) for far in _far_points(anchor, fan, ray_length)]
    counts = [len(fan) for fan in angles]
    if not fars:
        return [(np.zeros((0, 2)), np.zeros(0)) for _ in counts]
    index = np.repeat(np.arange(len(counts)), counts)
    hits, dist, _ = ray_hits(outlines, np.asarray(anchors, np.float64).reshape(-1, 2)[index], fars, index)
    cuts = np.cumsum(counts)[:-1]
    return list(zip(np.split(hits, cuts), np.split(dist, cuts)))


def get_ray_hitpoint(point_anchor, point_far, line_string, ret_dist=False):
    """the point where the ray from point_anchor to point_far first hits the outline line_string, as a tuple of
    floats, or None; with ret_dist (point, distance) or (None, nan).  Reference: video/analysis/regions.py:353-391;
    the definition is pinned in DESIGN.md §9, "Outline queries" (the hit of the smallest (t, edge); collinear
    overlaps do not count).  line_string: an (N, 2) array-like, an open line string as given (a ring repeats its
    first point); one of our Polygons, its contour closed; or an object with .coords."""
    hits, dist, edge = ray_hits([line_string], [point_anchor], [point_far])
    if edge[0] < 0:
        return (None, np.nan) if ret_dist else None
    point = (float(hits[0, 0]), float(hits[0, 1]))
    return (point, float(dist[0])) if ret_dist else point


def _ray_fan(point_anchor, angles, polygon, ray_length):
    """(hit point or None, distance) per angle: one launch, none without angles"""
    fars = _far_points(point_anchor, angles, ray_length)
    if not fars:
        return [], []
    hits, dist, edge = ray_hits([polygon], [point_anchor] * len(fars), fars)
    points = [(float(h[0]), float(h[1])) if e >= 0 else None for h, e in zip(hits, edge)]
    return points, dist.tolist()


def get_ray_intersections(point_anchor, angles, polygon, ray_length=1000):
    """the hit point (or None) of a ray from point_anchor at every angle, of length ray_length; one launch for the
    whole fan (reference: video/analysis/regions.py:395-405)"""
    return _ray_fan(point_anchor, angles, polygon, ray_length)[0]


def get_farthest_ray_intersection(point_anchor, angles, polygon, ray_length=1000):
    """(hit point, its distance from point_anchor, its angle) of the farthest hit of the fan, (None, 0, None)
    without one; a later ray replaces the best only on a strictly larger distance (reference:
    video/analysis/regions.py:409-426)"""
    points, dists = _ray_fan(point_anchor, angles, polygon, ray_length)
    point_max, dist_max, angle_max = None, 0, None
    for point, dist, angle in zip(points, dists, angles):
        if dist > dist_max:
            point_max, dist_max, angle_max = point, dist, angle
    return point_max, dist_max, angle_max
