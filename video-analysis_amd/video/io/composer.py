"""Composing an annotated video frame by frame (the reference's `video/io/composer.py`), batched on the GPU.

`VideoComposer` keeps the reference's method names and argument lists.  What differs, and why:

* **File name or sink.**  The reference is a `VideoFileWriter`; here the first argument is a file name (a `str` or
  `os.PathLike`), for which a `video.io.file.VideoFileWriter(filename, self.size, fps, is_color, **kwargs)` is
  opened and closed with the composer, or a *sink*: ``None`` collects the frames (``.frames`` returns them as an
  array fit for `VideoMemory`), an object with ``write_frame(frame)`` receives them, and so does a plain callable.
  A sink with ``write_frames(stack)`` -- the file writer is one -- receives a flush's finished frames as one
  `ops.DeviceFrames` where the flush needs no host copy of them: only what the sink makes of them crosses to the
  host (for the file writer the compressed bytes).  The stack is the composer's: the sink uses it during the call.
* **Deferred drawing.**  Calls are recorded per output frame and carried out for `batch` output frames at a time
  (default 32), on `close()`, and when `.frame` is read.  Everything a call is given is captured at call time, so a
  caller may reuse its arrays.  The order of the calls within a frame is kept: consecutive pixel layers
  (`highlight_mask`, `add_image`, `blend_image`) are one `ops.compose_layers` launch over all pending frames and
  consecutive drawing calls one `ops.draw` launch; a frame that alternates costs one pair per alternation.  The stack
  stays on the device in between: a flush is one upload and one download of the frames.
* **Zoom.**  Frames, images and masks go through `ops.resize` (linear, as ``cv2.resize(x, self.size)``);
  coordinates follow the reference's host expressions ``(points / zoom).astype(int)``, ``int(pos / zoom)`` and
  ``int(np.ceil(radius / zoom))``.  The reference's ``if mask:`` in `_prepare_images` raises for array masks; here
  the mask is resized as ``mask.astype(np.uint8)`` and taken as non-zero.
* **add_contour given a mask** finds the outer contours of all such masks of a flush with one `ops.find_contours`
  call.
* **add_line** splits at the reference's ``points[:, 0] > 0`` test into maximal runs of true entries
  (`contiguous_true_regions`, which the checkout lacks and which is restated here).
* **Limits.**  Thickness 1 only (OpenCV draws thicker primitives as filled polygons with round caps), no
  anti-aliased lines and no `add_text` (Hershey fonts): each raises `NotImplementedError`.  With the reference's
  defaults every call stays inside the supported set, for any zoom factor >= 1.

* **Whole stacks.**  `annotate_frames` (not in the reference) composes the common annotation -- highlight the mask,
  outline the blobs -- for a stack of frames in one call, from arrays or from stacks that are already on the device
  (`ops.DeviceFrames` of a decoder or of `FrameEngine.run(..., keep=("mask",))`, an `ops.DeviceContours`): with a
  `write_frames` sink nothing but what the sink makes of the frames leaves the device.

The ops are looked up on `video.ops` when a flush runs (`ops.compose_layers`, `ops.draw`, `ops.resize`,
`ops.find_contours`, and for `annotate_frames` `ops.draw_contours`, `ops.DeviceFrames` and `ops.DeviceContours`), so a
test can put other implementations in their place with `monkeypatch.setattr(ops, ...)`.
The pinned definitions are in DESIGN.md §9, "Composer" and "Annotating on the device".
"""
import math
import os

import numpy as np

from .. import ops
from ..analysis.regions import rect_to_corners

CHANNEL_NAMES = dict(ops.COMPOSE_CHANNELS)

# matplotlib's single-letter colours and the two names a tracker uses, for a machine without matplotlib
_BASE_COLORS = {"b": (0.0, 0.0, 1.0), "g": (0.0, 0.5, 0.0), "r": (1.0, 0.0, 0.0), "c": (0.0, 0.75, 0.75),
                "m": (0.75, 0.0, 0.75), "y": (0.75, 0.75, 0.0), "k": (0.0, 0.0, 0.0), "w": (1.0, 1.0, 1.0),
                "white": (1.0, 1.0, 1.0), "black": (0.0, 0.0, 0.0)}


def _table_parser(color):
    if isinstance(color, str):
        try:
            return _BASE_COLORS[color.lower()]
        except KeyError:
            raise ValueError("Unknown color %r (without matplotlib only %s are known)"
                             % (color, ", ".join(sorted(_BASE_COLORS))))
    rgb = tuple(float(c) for c in color)[:3]
    if len(rgb) != 3 or not all(0 <= c <= 1 for c in rgb):
        raise ValueError("RGB colors are three floats in 0 .. 1, got %r" % (color,))
    return rgb


def get_color(color):
    """an RGB color with channels ranging from 0..255, in matplotlib's color notation (its ColorConverter when
    matplotlib can be imported, else the single-letter names, 'white', 'black' and RGB tuples of floats)"""
    if get_color.parser is None:
        try:
            from matplotlib.colors import ColorConverter
            get_color.parser = ColorConverter().to_rgb
        except ImportError:
            get_color.parser = _table_parser
    return [int(255 * c) for c in get_color.parser(color)]


get_color.parser = None


def contiguous_true_regions(condition):
    """[(start, end)] of the maximal runs of true entries of a 1-d condition (end exclusive)"""
    cond = np.concatenate([[False], np.asarray(condition, bool), [False]])
    edges = np.flatnonzero(cond[1:] != cond[:-1])
    return [(int(a), int(b)) for a, b in zip(edges[::2], edges[1::2])]


def skip_if_no_output(func):
    """decorator which only calls the function if the current frame will be written"""
    def func_wrapper(self, *args, **kwargs):
        if self.output_this_frame:
            return func(self, *args, **kwargs)
    func_wrapper.__name__, func_wrapper.__doc__ = func.__name__, func.__doc__
    return func_wrapper


def _unsupported_thickness(thickness, what):
    raise NotImplementedError("%s: only thickness 1 is supported on the GPU path, got %r (OpenCV draws thicker "
                              "primitives as filled polygons with round caps)" % (what, thickness))


class _Pending(object):
    """one output frame that is not composed yet: the frame as it was handed in (or, `final`, as an earlier flush
    left it) and the recorded steps"""

    def __init__(self, image):
        self.image, self.final, self.steps = image, False, []


class VideoComposer(object):
    """A class that can be used to compose a video frame by frame; geometric objects and overlays can be added to
    each frame.  See the module's docstring for the differences from the reference."""

    def __init__(self, sink, size, fps, is_color, output_period=1, zoom_factor=1, batch=32, **kwargs):
        """`sink`: a file name, None, an object with write_frame(frame), or a callable.  `size` = (width, height) of
        the frames handed to set_frame; the output is (int(width / zoom_factor), int(height / zoom_factor)).
        `output_period`: only every output_period-th frame is written.  `batch`: output frames composed per flush.
        Further keyword arguments go to the file writer that a file name opens."""
        if batch < 1:
            raise ValueError("batch must be positive")
        self.sink, self.fps, self.is_color = sink, fps, bool(is_color)
        self.next_frame = -1
        self.output_period = output_period
        self.zoom_factor = zoom_factor
        self.source_size = (int(size[0]), int(size[1]))
        self.size = (int(size[0] / zoom_factor), int(size[1] / zoom_factor))
        self.batch = int(batch)
        self.frames_written = 0
        self._pending = []
        self._collected = []
        self._last_capture = {}
        if isinstance(sink, (str, os.PathLike)):
            from .file import VideoFileWriter
            self.sink = VideoFileWriter(sink, self.size, fps, self.is_color, **kwargs)

    # ------------------------------------------------------------------------------------------ bookkeeping
    def get_color(self, color):
        """takes the color and converts it into a usable representation"""
        color = get_color(color)
        if not self.is_color:
            color = int(np.mean(color))       # turn into grey scale
        return color

    @property
    def output_this_frame(self):
        """determines whether the current frame should be written to the video"""
        return (self.next_frame % self.output_period) == 0

    @property
    def frame(self):
        """the current frame as composed so far (this carries out everything recorded)"""
        if not self._pending:
            return None
        self._flush(keep_last=True)
        return self._pending[-1].image

    @property
    def frames(self):
        """the frames written so far to the sink None, as one (n, h, w[, 3]) uint8 array"""
        if self.sink is not None:
            raise AttributeError("frames are collected only with sink=None")
        shape = (0, self.size[1], self.size[0]) + ((3,) if self.is_color else ())
        return np.array(self._collected, np.uint8) if self._collected else np.zeros(shape, np.uint8)

    def _capture(self, array, as_mask=False):
        """a private uint8 copy of what a call was given, made once: the one copy of an array that has not changed
        since is shared between calls, so that a background image blended into every frame is captured once and
        uploaded once per flush.  The cache is keyed on the caller's own array object.  as_mask: the copy is the
        mask's non-zero pattern (a boolean mask is copied as its bytes, another dtype compared with 0 once).
        Whether a cached array has changed is seen by comparing it with its copy, which reads it once and writes
        nothing; an array that is read-only and owns its memory cannot have changed and is not compared."""
        array = np.asarray(array)
        last = self._last_capture.get(id(array))
        if last is not None and last[0] is array and last[1].shape == array.shape:
            frozen = not array.flags.writeable and array.base is None
            if frozen or np.array_equal(last[1], array if last[1].dtype == array.dtype else array != 0):
                return last[2]
        if as_mask and array.dtype not in (np.uint8, np.bool_):
            kept = array != 0                     # the one conversion; it is the private copy as well
        else:
            kept = np.array(array, copy=True)
        copy = kept.view(np.uint8) if kept.dtype == np.bool_ else kept
        if len(self._last_capture) > 8:
            self._last_capture.clear()
        self._last_capture[id(array)] = (array, kept, copy)
        return copy

    def _record(self, kind, item):
        if not self._pending:
            raise RuntimeError("there is no current frame: call set_frame first")
        self._pending[-1].steps.append((kind, item))

    # ------------------------------------------------------------------------------------------ frames
    def set_frame(self, frame, copy=True):
        """set the current frame from an image (always copied: the drawing is deferred)"""
        self.next_frame += 1
        if not self.output_this_frame:
            return
        frame = np.asarray(frame)
        if frame.dtype != np.uint8:
            raise TypeError("frames are uint8, got %s" % frame.dtype)
        if not self.is_color and frame.ndim == 3:
            raise ValueError("Cannot copy a color image into a monochrome video.")
        if not (frame.ndim == 2 or (frame.ndim == 3 and frame.shape[2] == 3)):
            raise ValueError("frames are (h, w) or (h, w, 3), got shape %r" % (frame.shape,))
        if frame.shape[:2] != (self.source_size[1], self.source_size[0]):
            raise ValueError("a frame of shape %r in a video of size %r" % (frame.shape, self.source_size))
        if len(self._pending) >= self.batch:
            self._flush(keep_last=False)
        self._pending.append(_Pending(np.array(frame, copy=True)))

    # ------------------------------------------------------------------------------------------ pixel layers
    def _layer_mask(self, mask):
        if mask is None:
            return None
        mask = np.asarray(mask)
        if mask.shape != (self.source_size[1], self.source_size[0]):
            raise ValueError("a mask of shape %r in a video of size %r" % (mask.shape, self.source_size))
        return self._capture(mask, as_mask=True)

    def _layer_image(self, image):
        image = np.asarray(image)
        if image.dtype != np.uint8:
            raise TypeError("images are uint8, got %s" % image.dtype)
        if image.shape[:2] != (self.source_size[1], self.source_size[0]) or image.ndim not in (2, 3):
            raise ValueError("The two images to be added must have the same size")
        if image.ndim == 3 and not self.is_color:
            raise ValueError("Cannot add a color image to a monochrome one")
        return self._capture(image)

    def _highlight_args(self, channel, strength):
        """the checked (channel, strength) of a highlight: the channel's index, or None for all"""
        if channel is None or (isinstance(channel, str) and channel == "all"):
            channel = None
        elif self.is_color:
            try:
                channel = CHANNEL_NAMES[channel]
            except (KeyError, TypeError):
                raise ValueError("Unknown value `%s` for channel." % (channel,))
        else:
            raise ValueError("Highlighting a specific channel is only supported for color videos.")
        if isinstance(strength, (bool, np.bool_)) or int(strength) != strength or not 0 <= strength <= 255:
            raise ValueError("the strength is an integer in 0 .. 255, got %r" % (strength,))
        return channel, int(strength)

    @skip_if_no_output
    def highlight_mask(self, mask, channel="all", strength=128):
        """highlights the non-zero entries of a mask in the current frame"""
        channel, strength = self._highlight_args(channel, strength)
        self._record("layer", ("highlight", self._layer_mask(mask), channel, strength))

    @skip_if_no_output
    def add_image(self, image, mask=None):
        """adds an image to the frame"""
        self._record("layer", ("add", self._layer_image(image), self._layer_mask(mask)))

    @skip_if_no_output
    def blend_image(self, image, weight=0.5, mask=None):
        """overlay image with weight"""
        weight = float(weight)
        if not math.isfinite(weight):
            raise ValueError("the weight must be finite, got %r" % weight)
        self._record("layer", ("blend", self._layer_image(image), weight, self._layer_mask(mask)))

    # ------------------------------------------------------------------------------------------ drawing
    def _zoom_points(self, points):
        """the reference's (points / zoom).astype(int); integer points go unchanged without a zoom"""
        points = np.asarray(points)
        if self.zoom_factor != 1:
            points = np.asarray(points, np.double) / self.zoom_factor
        return _checked_points(points.astype(np.int64))

    def _thickness(self, value, what):
        thickness = int(np.ceil(value / self.zoom_factor)) if self.zoom_factor != 1 else int(value)
        if thickness != 1:
            _unsupported_thickness(thickness, what)

    @skip_if_no_output
    def add_contour(self, mask_or_contour, color="w", thickness=1, copy=True):
        """adds the contours of a mask, of one contour or of a list of contours (the mask is never modified)"""
        self._thickness(thickness, "add_contour")
        color = self.get_color(color)
        if isinstance(mask_or_contour, list):
            contours = mask_or_contour
        elif any(s == 1 for s in np.shape(mask_or_contour)[:2]):
            contours = [mask_or_contour]
        else:
            mask = np.asarray(mask_or_contour)
            if mask.ndim != 2:
                raise ValueError("a mask is 2-dimensional, got shape %r" % (mask.shape,))
            self._record("mask_contours", (self._capture(mask, as_mask=True), color))
            return
        for c in contours:
            self._record("draw", ("polyline", self._zoom_points(np.asarray(c).reshape(-1, 2)), True, color))

    @skip_if_no_output
    def add_line(self, points, color="w", is_closed=True, mark_points=False, width=1):
        """adds a polygon to the frame"""
        if len(points) == 0:
            return
        self._thickness(width, "add_line")
        points = np.asarray(points)
        rgb = self.get_color(color)
        # the regions where the points are finite: comparing to 0 also catches the nans of an int32 array
        for start, end in contiguous_true_regions(points[:, 0] > 0):
            self._record("draw", ("polyline", self._zoom_points(points[start:end, :]), bool(is_closed), rgb))
            if mark_points:
                for p in points[start:end, :]:
                    self.add_circle(p, 2 * width, color, thickness=-1)

    @skip_if_no_output
    def add_rectangle(self, rect, color="w", width=1):
        """add a rect=(left, top, width, height) to the frame"""
        self._thickness(width, "add_rectangle")
        if self.zoom_factor != 1:
            rect = np.asarray(rect) / self.zoom_factor
        try:
            corners = rect.corners
        except AttributeError:
            corners = rect_to_corners(rect)
        (x1, y1), (x2, y2) = [(int(p[0]), int(p[1])) for p in corners]
        points = _checked_points(np.array([(x1, y1), (x2, y1), (x2, y2), (x1, y2)], np.int64))
        self._record("draw", ("polyline", points, True, self.get_color(color)))

    @skip_if_no_output
    def add_circle(self, pos, radius=2, color="w", thickness=-1):
        """add a circle to the frame; thickness=-1 denotes a filled circle"""
        if thickness == 0:
            raise NotImplementedError("add_circle: thickness 0 is not a circle OpenCV draws")
        if thickness > 0:
            self._thickness(thickness, "add_circle")
        try:
            pos = (int(pos[0] / self.zoom_factor), int(pos[1] / self.zoom_factor))
            radius = int(np.ceil(radius / self.zoom_factor))
        except (ValueError, OverflowError):
            return
        if max(abs(pos[0]), abs(pos[1]), abs(radius)) > ops.DRAW_MAX_COORD:
            return                             # (the reference's cv2 call raises OverflowError here, and is skipped)
        self._record("draw", ("circle", pos, radius, thickness < 0, self.get_color(color)))

    @skip_if_no_output
    def add_points(self, points, radius=1, color="w"):
        """adds a sequence of points to the frame"""
        for p in points:
            self.add_circle(p, radius, color, thickness=-1)

    @skip_if_no_output
    def add_text(self, text, pos, color="w", size=1, anchor="bottom", font=None):
        raise NotImplementedError("add_text: text needs OpenCV's Hershey font tables, which this package does not "
                                  "carry; no text is drawn on the GPU path")

    # ------------------------------------------------------------------------------------------ flushing
    def _write(self, frame):
        self.frames_written += 1
        if self.sink is None:
            self._collected.append(frame)
        elif hasattr(self.sink, "write_frame"):
            self.sink.write_frame(frame)
        else:
            self.sink(frame)

    def _frame_shape(self):
        return (self.size[1], self.size[0]) + ((3,) if self.is_color else ())

    def _resized(self, arrays, color):
        """ops.resize (linear) of every array of a list to self.size, one call per shape"""
        out, groups = [None] * len(arrays), {}
        for i, a in enumerate(arrays):
            groups.setdefault(a.shape, []).append(i)
        for idx in groups.values():
            res = ops.resize(np.stack([arrays[i] for i in idx]), self.size, "linear", color=color)
            for i, r in zip(idx, res):
                out[i] = r
        return out

    def _prepare(self, pending):
        """frames, images and masks at the output geometry (the zoom), and the contours of the recorded masks:
        returns the host stack and, per frame, the steps as ('layer' | 'draw', item)"""
        zoom = self.zoom_factor != 1
        images = [p.image for p in pending]
        raw = [i for i, p in enumerate(pending) if not p.final]
        if zoom and raw:
            for color in (False, True):
                idx = [i for i in raw if (images[i].ndim == 3) == color]
                for i, r in zip(idx, self._resized([images[i] for i in idx], color)):
                    images[i] = r
        if len({im.ndim for im in images}) > 1:               # monochrome and colour frames in one flush
            images = [np.repeat(im[:, :, None], 3, axis=2) if im.ndim == 2 else im for im in images]
        stack = np.stack(images)
        # the distinct images and masks of the layers, resized once each
        sized = {}
        if zoom:
            planes = {}
            for p in pending:
                for kind, item in p.steps:
                    if kind == "layer":
                        for a in item[1:]:
                            if isinstance(a, np.ndarray):
                                planes[id(a)] = a
            keys = list(planes)
            for color in (False, True):
                idx = [k for k in keys if (planes[k].ndim == 3) == color]
                src = [planes[k].astype(np.uint8) if planes[k].dtype != np.uint8 else planes[k] for k in idx]
                for k, r in zip(idx, self._resized(src, color) if idx else []):
                    sized[k] = r
        # the contours of the recorded masks: one find_contours call per mask shape
        todo = [(f, s) for f, p in enumerate(pending) for s, (kind, _) in enumerate(p.steps) if kind == "mask_contours"]
        found, groups = {}, {}
        for f, s in todo:
            groups.setdefault(pending[f].steps[s][1][0].shape, []).append((f, s))
        for where in groups.values():
            masks = np.stack([pending[f].steps[s][1][0] for f, s in where])
            for key, contours in zip(where, ops.find_contours(masks)):
                found[key] = contours
        steps = []
        for f, p in enumerate(pending):
            mine = []
            for s, (kind, item) in enumerate(p.steps):
                if kind == "layer":
                    mine.append(("layer", tuple(sized.get(id(a), a) if isinstance(a, np.ndarray) else a
                                                for a in item)))
                elif kind == "draw":
                    mine.append(("draw", item))
                else:
                    for c in found[(f, s)]:
                        mine.append(("draw", ("polyline", self._zoom_points(c.reshape(-1, 2)), True, item[1])))
            steps.append(mine)
        return stack, steps

    def _flush(self, keep_last):
        """carry out everything recorded; write the finished frames (all, or all but the current one) to the sink"""
        pending = self._pending
        if not pending:
            return
        if any(p.steps or not p.final for p in pending):
            stack, steps = self._prepare(pending)
            # alternating runs per frame, starting with the layers: round 2k is a compose pass, 2k + 1 a draw pass
            runs = []
            for mine in steps:
                r = [[]]
                for kind, item in mine:
                    if (kind == "draw") != (len(r) % 2 == 0):
                        r.append([])
                    r[-1].append(item)
                runs.append(r)
            current = stack
            # a sink that takes stacks gets the device stack itself when every frame of it is written now (nothing
            # is kept for .frame): no host copy of the frames is needed then
            direct = not keep_last and hasattr(self.sink, "write_frames")
            try:
                for k in range(max(len(r) for r in runs)):
                    items = [r[k] if k < len(r) else [] for r in runs]
                    if k % 2 == 0:
                        if k == 0 or any(items):
                            current = ops.compose_layers(current, items, color=self.is_color, keep=True)
                    elif any(items):
                        current = ops.draw(current, items, keep=True)
                if direct and isinstance(current, ops.DeviceFrames) and current.shape[1:] == self._frame_shape():
                    self.sink.write_frames(current)
                    self.frames_written += len(pending)
                    self._pending = []
                    return
                out = current.download() if hasattr(current, "download") else np.asarray(current)
            finally:
                if hasattr(current, "release"):
                    current.release()
            for p, image in zip(pending, out):
                p.image, p.final, p.steps = image, True, []
        done = pending[:-1] if keep_last else pending
        self._pending = pending[-1:] if keep_last else []
        for p in done:
            self._write(p.image)

    # ------------------------------------------------------------------------------------------ whole stacks
    def annotate_frames(self, frames, masks=None, channel="all", strength=128, contours=None, color="w"):
        """A whole stack of `n` source frames at once, with the result of this loop, byte for byte:

            for i in range(n):
                composer.set_frame(frames[i])
                if masks is not None:    composer.highlight_mask(masks[i], channel, strength)
                if contours is not None: composer.add_contour(<the contours of frame i>, color)

        frames: an (n, h, w[, 3]) uint8 array or an `ops.DeviceFrames`; masks: an (n, h, w) array or a monochrome
        `ops.DeviceFrames`; contours: an `ops.DeviceContours` of the same `n` frames, or True for the outer contours
        of `masks` (one `ops.find_contours(..., keep=True)`), or None.  What is handed in is not modified and stays
        the caller's.  With stacks that are on the device, nothing crosses to the host but what the sink makes of
        the finished frames: a sink with ``write_frames`` receives them as one `ops.DeviceFrames` (the composer's,
        for the duration of the call); any other sink gets a download.

        Pending per-frame work is flushed first, so the output order is the call order; `next_frame` advances by
        `n`; with `output_period != 1` only the frames the loop would write are composed (gathered on the device,
        their contours selected through a frame map).  Afterwards there is no current frame until the next
        `set_frame`.  The checks of `set_frame`, `highlight_mask` and `get_color` apply as in the loop: none when no
        frame of the stack is written.  `zoom_factor != 1` raises NotImplementedError."""
        if self.zoom_factor != 1:
            raise NotImplementedError("annotate_frames: zoom_factor %r is not supported on whole stacks, only 1 "
                                      "(ops.resize has no device-resident form)" % (self.zoom_factor,))
        on_device = isinstance(frames, ops.DeviceFrames)
        if not on_device:
            frames = np.asarray(frames)
        if len(frames.shape) < 1:
            raise ValueError("frames are a stack (n, h, w) or (n, h, w, 3), got shape %r" % (frames.shape,))
        n = frames.shape[0]
        chosen = [i for i in range(n) if (self.next_frame + 1 + i) % self.output_period == 0]
        if not chosen:
            self.next_frame += n
            return
        if not on_device and frames.dtype != np.uint8:
            raise TypeError("frames are uint8, got %s" % frames.dtype)
        shape = tuple(frames.shape)
        if not self.is_color and len(shape) == 4:
            raise ValueError("Cannot copy a color image into a monochrome video.")
        if not (len(shape) == 3 or (len(shape) == 4 and shape[3] == 3)):
            raise ValueError("frames are a stack (n, h, w) or (n, h, w, 3), got shape %r" % (shape,))
        size = (self.source_size[1], self.source_size[0])
        if shape[1:3] != size:
            raise ValueError("frames of shape %r in a video of size %r" % (shape, self.source_size))
        masks_on_device = isinstance(masks, ops.DeviceFrames)
        if masks is not None:
            if not masks_on_device:
                masks = np.asarray(masks)
            if tuple(masks.shape) != (n,) + size:
                raise ValueError("masks of shape %r for %d frames in a video of size %r"
                                 % (tuple(masks.shape), n, self.source_size))
            channel, strength = self._highlight_args(channel, strength)
        if contours is not None:
            if contours is True:
                if masks is None:
                    raise ValueError("contours=True finds the contours of the masks: there are none")
            elif not isinstance(contours, ops.DeviceContours):
                raise TypeError("contours are an ops.DeviceContours, True or None, got %s" % type(contours).__name__)
            elif (contours.n, contours.h, contours.w) != (n,) + size:
                raise ValueError("contours of %d frames of %r for %d frames of %r"
                                 % (contours.n, (contours.h, contours.w), n, size))
            color = self.get_color(color)
        self._flush(keep_last=False)
        self.next_frame += n
        whole = len(chosen) == n
        own = []                                  # what this call has put on the device
        current = None
        try:
            # the frames that are written, as a stack of the composer's own
            if on_device:
                current = frames.gather(chosen)
            else:
                current = ops.DeviceFrames.upload(frames if whole else frames[chosen])
            # their masks: planes of the caller's stack, or an upload of the chosen ones' non-zero patterns
            planes = None
            if masks is not None:
                if masks_on_device:
                    mask_stack, planes = masks, chosen
                else:
                    picked = masks if whole else masks[chosen]
                    bits = picked if picked.dtype == np.uint8 else (picked != 0).view(np.uint8)
                    mask_stack, planes = ops.DeviceFrames.upload(bits), list(range(len(chosen)))
                    own.append(mask_stack)
            # their contours, and the map from the frames these were found in to the frames of `current`
            frame_map = None
            if contours is True:
                contours = ops.find_contours(mask_stack, keep=True)
                own.append(contours)
                if masks_on_device and not whole:
                    frame_map = np.full(n, -1, np.int32)
                    frame_map[chosen] = np.arange(len(chosen), dtype=np.int32)
            elif contours is not None and not whole:
                frame_map = np.full(n, -1, np.int32)
                frame_map[chosen] = np.arange(len(chosen), dtype=np.int32)
            layers = [[("highlight", (mask_stack, k), channel, strength)] if planes is not None else []
                      for k in (planes if planes is not None else chosen)]
            current = ops.compose_layers(current, layers, color=self.is_color, keep=True)
            if contours is not None:
                current = ops.draw_contours(current, contours, color, frame_map=frame_map, keep=True)
            if hasattr(self.sink, "write_frames"):
                self.sink.write_frames(current)
                self.frames_written += len(chosen)
            else:
                for image in current.download():
                    self._write(image)
        finally:
            for held in own + ([current] if current is not None else []):
                held.release()

    def close(self):
        """compose and write what is pending"""
        self._flush(keep_last=False)
        self._last_capture.clear()
        if self.sink is not None and hasattr(self.sink, "write_frame") and hasattr(self.sink, "close"):
            self.sink.close()


def _checked_points(points):
    if points.size and np.abs(points).max() > ops.DRAW_MAX_COORD:
        raise ValueError("a coordinate is beyond +-%d" % ops.DRAW_MAX_COORD)
    return points


class VideoComposerListener(VideoComposer):
    """A composer that listens to another video and captures every frame that video hands out; geometric objects
    can then be added to each frame.  This is useful to annotate a copy of a video.  (Listeners see the frames that
    pass a video's `_process_frame`, that is the frames of filters; a bare `VideoMemory` hands out views of its array
    without it, so wrap it in a filter, `VideoFilterBase(memory)` at the least.)"""

    def __init__(self, sink, background_video, is_color=None, **kwargs):
        self.background_video = background_video
        self.background_video.register_listener(self.set_frame)
        if is_color is None:
            is_color = background_video.is_color
        super(VideoComposerListener, self).__init__(sink, self.background_video.size, self.background_video.fps,
                                                    is_color, **kwargs)

    def close(self):
        try:
            self.background_video.unregister_listener(self.set_frame)
        except (AttributeError, ValueError):
            pass                               # apparently, the listener is already removed
        super(VideoComposerListener, self).close()
