"""Tracks from region links: which region of a frame continues which region of the frame before.

The reference has no tracker of regions; this is the consumer of `FrameEngine.run(..., want=(..., "links"))` and of
`ops.region_links` ("Region links"): host arithmetic with NumPy on the small link tables.  The label
planes themselves never leave the device.

`TemplateTracker` is the second way to follow objects, for where blobs touch, rest or the camera moves: template
matching in a window around each object's last position (`ops.match_templates`; DESIGN.md §9, "Template matching").
"""
import collections

import numpy as np

Tracks = collections.namedtuple("Tracks", "ids counts stats links_in links_out")


def _best(keys, partners, counts, size):
    """per key 1 .. size the partner with the largest count, ties to the smallest partner; 0 without a link"""
    best = np.zeros(size + 1, np.int64)
    order = np.lexsort((partners, -counts, keys))         # by key, then count descending, then partner ascending
    k = keys[order]
    lead = np.ones(k.size, bool)
    lead[1:] = k[1:] != k[:-1]
    best[k[lead]] = partners[order][lead]
    return best


class RegionTracker(object):
    """track ids for the regions of consecutive frames from their overlap links.

    A link (a, b, count) says that `count` pixels of region a of the earlier frame lie in region b of the later one;
    links with count < min_overlap do not exist.  succ(a) is the b with the largest count among the links out of a,
    pred(b) the a with the largest count among the links into b, ties going to the smallest label.  Region b
    continues the track of a iff b = succ(a) and a = pred(b); every other region starts a track with the next new
    id.  Ids are consecutive from 0 and handed out in (frame, label) order.  The tracker keeps the ids of the last
    frame it saw: the links of frame 0 of an update refer to that frame."""

    def __init__(self, min_overlap=1):
        self.min_overlap = int(min_overlap)
        self.next_id = 0
        self.last_ids = None            # the ids of the last frame seen; None before the first

    def update(self, links, counts):
        """links: an ops.RegionLinks (or any (offsets, a, b, count)) of n frames; counts: the regions of each frame,
        labels 1 .. counts[t].  Returns (ids, links_in, links_out), one int64 array per frame each:
        ids[t][label - 1] is the track id of the region; links_in[t][label - 1] the number of links into it (0: a
        birth, 2 or more: a merge); links_out[t][label - 1] the number of links out of that region of the earlier
        frame of pair t (0: a death, 2 or more: a split; empty for a first frame).  Links of frame 0 without an
        earlier frame are a ValueError, as is a label outside 1 .. counts."""
        offsets, la, lb, lc = (np.asarray(v) for v in links)
        counts = np.asarray(counts).reshape(-1)
        if offsets.size != counts.size + 1:
            raise ValueError("links of %d frames, counts of %d" % (offsets.size - 1, counts.size))
        ids, links_in, links_out = [], [], []
        for t in range(counts.size):
            sl = slice(int(offsets[t]), int(offsets[t + 1]))
            a, b, c = la[sl].astype(np.int64), lb[sl].astype(np.int64), lc[sl].astype(np.int64)
            nb = int(counts[t])
            if self.last_ids is None:
                if a.size:
                    raise ValueError("frame %d has links but the tracker has seen no earlier frame" % t)
                na = 0
            else:
                na = self.last_ids.size
            if a.size and (a.min() < 1 or a.max() > na or b.min() < 1 or b.max() > nb):
                raise ValueError("frame %d: a link names a label outside 1 .. %d -> 1 .. %d" % (t, na, nb))
            real = c >= self.min_overlap
            a, b, c = a[real], b[real], c[real]
            succ, pred = _best(a, b, c, na), _best(b, a, c, nb)
            labels = np.arange(1, nb + 1)
            carried = pred[labels] > 0
            carried[carried] = succ[pred[labels[carried]]] == labels[carried]
            new = np.empty(nb, np.int64)
            if carried.any():
                new[carried] = self.last_ids[pred[labels[carried]] - 1]
            born = int(nb - carried.sum())
            new[~carried] = self.next_id + np.arange(born)
            self.next_id += born
            self.last_ids = new
            ids.append(new)
            links_in.append(np.bincount(b, minlength=nb + 1)[1:].astype(np.int64))
            links_out.append(np.bincount(a, minlength=na + 1)[1:].astype(np.int64))
        return ids, links_in, links_out


def track_regions(engine, frames, batch=None):
    """the regions of a whole clip and their track ids: runs `engine` (a FrameEngine that labels) over `frames` in
    batches of `batch` (default: its max_batch) with want=('counts', 'stats', 'links') -- 'stats' where the engine
    has max_labels -- and feeds a RegionTracker.  frames: an (n, H, W[, C]) array or an ops.DeviceFrames.  Only
    counts, statistics and link tables cross to the host, no label plane.  Returns Tracks(ids, counts, stats,
    links_in, links_out): ids, links_in, links_out as RegionTracker.update returns them, counts (n,) int32,
    stats a list of (counts[t], 16) int64 arrays (None without max_labels)."""
    from .. import ops
    batch = int(batch or engine.max_batch)
    if not 1 <= batch <= engine.max_batch:
        raise ValueError("batch of %d, the engine takes 1 .. %d" % (batch, engine.max_batch))
    want = ("counts", "stats", "links") if engine.max_labels > 0 else ("counts", "links")
    resident = isinstance(frames, ops.DeviceFrames)
    n = frames.n if resident else len(frames)
    engine.reset_links()
    tracker = RegionTracker()
    ids, lin, lout, counts, stats = [], [], [], [], []
    for first in range(0, n, batch):
        last = min(first + batch, n)
        if resident:
            part = frames.gather(range(first, last))
            try:
                out = engine.run_frames(part, want=want)
            finally:
                part.release()
        else:
            out = engine.run(frames[first:last], want=want)
        got = tracker.update(out["links"], out["counts"])
        for acc, new in zip((ids, lin, lout), got):
            acc.extend(new)
        counts.append(out["counts"])
        if "stats" in out:
            stats.extend(out["stats"][t, :min(int(k), engine.max_labels)] for t, k in enumerate(out["counts"]))
    return Tracks(ids, np.concatenate(counts) if counts else np.zeros(0, np.int32), stats if "stats" in want else None,
                  lin, lout)


class TemplateTracker(object):
    """follows k templates through batches of frames by template matching (ops.match_templates; DESIGN.md §9,
    "Template matching").

    templates: 2-d uint8 arrays; positions: (k, 2) integer (x, y) of their top-left corners in the frame before the
    first batch; radius: how far, in pixels along each axis, a template is looked for around its position.
    update(frames) asks one query per frame of the batch and template: the positions within `radius` of the template's
    position at the start of the batch, clipped to the frame (image.template_search_window).  So `radius` must cover
    the motion of a whole batch, not of one frame: choose the batch and the radius together.  The positions found in
    the last frame of a batch centre the next one.  A batch is one launch chain, and only the best records cross to
    the host.  The templates stay what they were given as: refreshing them from the frames is not built."""

    def __init__(self, templates, positions, radius, method="ccoeff_normed"):
        from .. import ops
        self.templates = ops._match_templates_in(list(templates), "TemplateTracker")
        self.positions = np.array(positions, np.int64).reshape(-1, 2)
        if len(self.positions) != len(self.templates) or not self.templates:
            raise ValueError("TemplateTracker: %d templates and %d positions" % (len(self.templates), len(self.positions)))
        if not (isinstance(radius, (int, np.integer)) and not isinstance(radius, bool) and radius >= 0):
            raise ValueError("TemplateTracker: the radius is an integer >= 0, got %r" % (radius,))
        if method not in ops.MATCH_METHODS:
            raise ValueError("TemplateTracker: method %r is not one of %s" % (method, sorted(ops.MATCH_METHODS)))
        self.radius, self.method = int(radius), method

    def queries(self, n, frame_shape):
        """the (n * k, 6) query table of a batch of n frames of `frame_shape` = (h, w), frame-major"""
        from .image import template_search_window
        r = self.radius
        windows = [template_search_window((x - r, y - r, 2 * r + t.shape[1], 2 * r + t.shape[0]), t.shape, frame_shape)
                   for t, (x, y) in zip(self.templates, self.positions.tolist())]
        return np.array([(f, k) + window for f in range(n) for k, window in enumerate(windows)],
                        np.int32).reshape(-1, 6)

    def update(self, frames):
        """frames: a monochrome uint8 stack (n, h, w) or an ops.DeviceFrames.  Returns (positions (n, k, 2) int32,
        scores (n, k) float64) and moves the tracker to the positions of the last frame."""
        from .. import ops
        k = len(self.templates)
        if isinstance(frames, ops.DeviceFrames):
            n, shape = frames.n, (frames.h, frames.w)
        else:
            frames = np.asarray(frames)
            if frames.dtype != np.uint8 or frames.ndim != 3:
                raise TypeError("TemplateTracker.update: frames are a monochrome uint8 stack (n, h, w), got %s of shape "
                                "%r" % (frames.dtype, frames.shape))
            n, shape = len(frames), frames.shape[1:]
        if n == 0:
            return np.zeros((0, k, 2), np.int32), np.zeros((0, k))
        best = ops.match_templates(frames, self.templates, self.queries(n, shape), method=self.method)
        positions = np.stack([best["x"], best["y"]], axis=1).reshape(n, k, 2)
        self.positions = positions[-1].astype(np.int64)
        return positions, best["score"].reshape(n, k).copy()
