"""NumPy restatement of DESIGN.md §9 "Composer", pixel by pixel (test infrastructure: the product package never
imports this file).

The line is restated from OpenCV's own formulation -- clipLine with its outcodes, then LineIterator's
err / plusDelta / minusDelta with a step that always moves along the major axis and moves along the minor one when
err < 0 -- not from the kernel's text; the circle is the recurrence of the section; the layers use explicit
np.float64 / np.float32 steps, one rounding each.

    compose_layers(frames, layers, color=None)      what ops.compose_layers computes
    draw(frames, commands)                          what ops.draw computes
    Replay                                          a VideoComposer call sequence, carried out frame by frame

compose_layers and draw take (and ignore) the keyword arguments of the ops, so that a test can put them in the
ops' place (tests/test_composer_host.py)."""
import math

import numpy as np

MAX_COORD = 1 << 20


# ------------------------------------------------------------------------------------------------ lines
def clip_line(w, h, x1, y1, x2, y2):
    """cv::clipLine(Size(w, h), pt1, pt2): (inside, x1, y1, x2, y2)"""
    if w <= 0 or h <= 0:
        return False, x1, y1, x2, y2
    right, bottom = w - 1, h - 1

    def code(x, y):
        return (x < 0) + (x > right) * 2 + (y < 0) * 4 + (y > bottom) * 8

    c1, c2 = code(x1, y1), code(x2, y2)
    if (c1 & c2) == 0 and (c1 | c2) != 0:
        if c1 & 12:
            a = 0 if c1 < 8 else bottom
            x1 += int(float(a - y1) * float(x2 - x1) / float(y2 - y1))      # int(): towards zero, as the C cast
            y1 = a
            c1 = (x1 < 0) + (x1 > right) * 2
        if c2 & 12:
            a = 0 if c2 < 8 else bottom
            x2 += int(float(a - y2) * float(x2 - x1) / float(y2 - y1))
            y2 = a
            c2 = (x2 < 0) + (x2 > right) * 2
        if (c1 & c2) == 0 and (c1 | c2) != 0:
            if c1:
                a = 0 if c1 == 1 else right
                y1 += int(float(a - x1) * float(y2 - y1) / float(x2 - x1))
                x1 = a
                c1 = 0
            if c2:
                a = 0 if c2 == 1 else right
                y2 += int(float(a - x2) * float(y2 - y1) / float(x2 - x1))
                x2 = a
                c2 = 0
    return (c1 | c2) == 0, x1, y1, x2, y2


def line_pixels(w, h, x1, y1, x2, y2):
    """the pixels of Line(img, p1, p2, color, 8): LineIterator(img, p1, p2, 8, leftToRight=True), in its order"""
    x1, y1, x2, y2 = int(x1), int(y1), int(x2), int(y2)
    if not (0 <= x1 < w and 0 <= x2 < w and 0 <= y1 < h and 0 <= y2 < h):
        ok, x1, y1, x2, y2 = clip_line(w, h, x1, y1, x2, y2)
        if not ok:
            return []
    dx, dy = x2 - x1, y2 - y1
    if dx < 0:                                   # leftToRight: iterate from the other end
        dx, dy, x1, y1 = -dx, -dy, x2, y2
    xstep, ystep = (1, 0), (0, 1 if dy >= 0 else -1)
    dy = abs(dy)
    if dy > dx:                                  # the major axis is y: the roles swap
        dx, dy = dy, dx
        xstep, ystep = ystep, xstep
    err, plus_delta, minus_delta = dx - (dy + dy), dx + dx, -(dy + dy)
    plus_step, minus_step, count = ystep, xstep, dx + 1
    out, x, y = [], x1, y1
    for _ in range(count):
        out.append((x, y))
        take = err < 0
        err += minus_delta + (plus_delta if take else 0)
        x += minus_step[0] + (plus_step[0] if take else 0)
        y += minus_step[1] + (plus_step[1] if take else 0)
    return out


def polyline_pixels(w, h, points, closed):
    """cv2.polylines(img, [points], closed, color, 1): the pixels of its segments"""
    v = np.asarray(points, np.int64).reshape(-1, 2)
    k = len(v)
    out = []
    for i in range(1, k):
        out += line_pixels(w, h, v[i - 1, 0], v[i - 1, 1], v[i, 0], v[i, 1])
    if closed and k:
        out += line_pixels(w, h, v[k - 1, 0], v[k - 1, 1], v[0, 0], v[0, 1])
    return out


# ------------------------------------------------------------------------------------------------ circles
def circle_pixels(w, h, cx, cy, r, filled):
    """OpenCV's integer Circle, intersected with the image: a list of (x, y), duplicates included"""
    out = []
    if r < 0:
        return out

    def put(x, y):
        if 0 <= x < w and 0 <= y < h:
            out.append((x, y))

    err, dx, dy, plus, minus = 0, r, 0, 1, 2 * r - 1
    while dx >= dy:
        if filled:
            for y, half in ((cy - dy, dx), (cy + dy, dx), (cy - dx, dy), (cy + dx, dy)):
                if 0 <= y < h:
                    for x in range(max(cx - half, 0), min(cx + half, w - 1) + 1):
                        out.append((x, y))
        else:
            for sx in (-1, 1):
                for sy in (-1, 1):
                    put(cx + sx * dx, cy + sy * dy)
                    put(cx + sx * dy, cy + sy * dx)
        dy += 1
        err += plus
        plus += 2
        if err > 0:
            err -= minus
            dx -= 1
            minus -= 2
    return out


# ------------------------------------------------------------------------------------------------ drawing
def draw_frame(frame, commands):
    """the commands of one frame, in list order, into `frame` (h, w) or (h, w, 3), in place"""
    h, w = frame.shape[:2]
    for cmd in commands:
        if cmd[0] == "polyline":
            _, points, closed, color = cmd
            pix = polyline_pixels(w, h, points, closed)
        elif cmd[0] == "circle":
            _, center, radius, filled, color = cmd
            pix = circle_pixels(w, h, int(center[0]), int(center[1]), int(radius), bool(filled))
        else:
            raise ValueError("unknown command %r" % (cmd[0],))
        for x, y in pix:
            frame[y, x] = color
    return frame


def draw(frames, commands, keep=False, stream=None):
    out = np.array(frames, np.uint8, copy=True)
    for f in range(len(out)):
        draw_frame(out[f], commands[f])
    return out


# ------------------------------------------------------------------------------------------------ layers
CHANNELS = {0: 0, "r": 0, "red": 0, 1: 1, "g": 1, "green": 1, 2: 2, "b": 2, "blue": 2}


def highlight(frame, mask, channel, strength):
    """composer.py:131-154: the masked pixels become trunc(strength + factor * v) in float64"""
    on = np.asarray(mask) != 0
    factor = np.float64(255 - strength) / np.float64(255)
    chans = [Ellipsis] if frame.ndim == 2 else ([0, 1, 2] if channel in (None, "all") else [CHANNELS[channel]])
    for ch in chans:
        plane = frame if ch is Ellipsis else frame[:, :, ch]
        t = np.float64(strength) + (factor * plane.astype(np.float64))           # product, then sum
        plane[on] = np.trunc(t).astype(np.uint8)[on]
    return frame


def _image_for(frame, image):
    image = np.asarray(image, np.uint8)
    if frame.ndim == 3 and image.ndim == 2:
        image = np.repeat(image[:, :, None], 3, axis=2)
    return image


def add(frame, image, mask):
    image = _image_for(frame, image)
    on = np.ones(frame.shape[:2], bool) if mask is None else np.asarray(mask) != 0
    s = np.minimum(frame.astype(np.int64) + image.astype(np.int64), 255).astype(np.uint8)
    frame[on] = s[on]
    return frame


def blend_values(v, u, weight):
    """cv2.addWeighted(v, 1 - w, u, w, 0) for uint8 as the section pins it"""
    alpha, beta = np.float32(1 - weight), np.float32(weight)
    a = (np.asarray(v).astype(np.float32) * alpha).astype(np.float32)
    b = (np.asarray(u).astype(np.float32) * beta).astype(np.float32)
    t = (a + b).astype(np.float32)
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)                  # np.rint: ties to even


def blend(frame, image, weight, mask):
    image = _image_for(frame, image)
    on = np.ones(frame.shape[:2], bool) if mask is None else np.asarray(mask) != 0
    r = blend_values(frame, image, weight)
    frame[on] = r[on]
    return frame


def compose_frame(frame, layers):
    for layer in layers:
        if layer[0] == "highlight":
            highlight(frame, layer[1], layer[2], layer[3])
        elif layer[0] == "add":
            add(frame, layer[1], layer[2])
        elif layer[0] == "blend":
            blend(frame, layer[1], layer[2], layer[3])
        else:
            raise ValueError("unknown layer %r" % (layer[0],))
    return frame


def compose_layers(frames, layers, color=None, keep=False, stream=None):
    frames = np.asarray(frames, np.uint8)
    if color is None:
        color = frames.ndim == 4
    if color and frames.ndim == 3:
        out = np.repeat(frames[:, :, :, None], 3, axis=3)
    else:
        out = frames.copy()
    for f in range(len(out)):
        compose_frame(out[f], layers[f])
    return out


# ------------------------------------------------------------------------------------------------ the composer
def contiguous_true_regions(cond):
    """[(start, end)] of the maximal runs of true entries"""
    runs, start = [], None
    for i, c in enumerate(list(cond) + [False]):
        if c and start is None:
            start = i
        elif not c and start is not None:
            runs.append((start, i))
            start = None
    return runs


class Replay(object):
    """a VideoComposer call sequence carried out at once, frame by frame, with the functions above; `resize` and
    `find_contours` are handed in (the zoom and add_contour(mask) steps are other ops, tested on their own)"""

    def __init__(self, size, is_color, output_period=1, zoom_factor=1, resize=None, find_contours=None,
                 get_color=None):
        self.is_color, self.period, self.zoom = is_color, output_period, zoom_factor
        self.size = (int(size[0] / zoom_factor), int(size[1] / zoom_factor))
        self.resize, self.find_contours, self._color = resize, find_contours, get_color
        self.out, self.frame, self.next = [], None, -1

    @property
    def on(self):
        return self.next % self.period == 0

    def color(self, c):
        rgb = self._color(c)
        return rgb if self.is_color else int(np.mean(rgb))

    def _sized(self, img, color):
        if self.zoom == 1:
            return np.array(img, np.uint8)
        return self.resize(np.asarray(img, np.uint8), self.size, "linear", color=color)

    def _mask(self, mask):
        if mask is None:
            return None
        if self.zoom == 1:
            return np.asarray(mask) != 0
        return self._sized(np.asarray(mask).astype(np.uint8), False) != 0

    def set_frame(self, frame):
        self.next += 1
        if not self.on:
            return
        if self.frame is not None:
            self.out.append(self.frame)
        frame = self._sized(frame, np.ndim(frame) == 3)
        if self.is_color and frame.ndim == 2:
            frame = np.repeat(frame[:, :, None], 3, axis=2)
        self.frame = frame

    def highlight_mask(self, mask, channel="all", strength=128):
        if self.on:
            highlight(self.frame, self._mask(mask), channel, strength)

    def add_image(self, image, mask=None):
        if self.on:
            add(self.frame, self._sized(image, np.ndim(image) == 3), self._mask(mask))

    def blend_image(self, image, weight=0.5, mask=None):
        if self.on:
            blend(self.frame, self._sized(image, np.ndim(image) == 3), weight, self._mask(mask))

    def add_contour(self, mask_or_contour, color="w"):
        if not self.on:
            return
        if isinstance(mask_or_contour, list):
            contours = mask_or_contour
        elif any(s == 1 for s in mask_or_contour.shape[:2]):
            contours = [mask_or_contour]
        else:
            contours = self.find_contours(mask_or_contour)
        for c in contours:
            c = np.asarray(c)
            if self.zoom != 1:
                c = (np.asarray(c, np.double) / self.zoom).astype(int)
            draw_frame(self.frame, [("polyline", c.reshape(-1, 2), True, self.color(color))])

    def add_line(self, points, color="w", is_closed=True, mark_points=False, width=1):
        if not self.on or len(points) == 0:
            return
        points = np.asarray(points)
        for start, end in contiguous_true_regions(points[:, 0] > 0):
            line = (points[start:end, :] / self.zoom).astype(int)
            draw_frame(self.frame, [("polyline", line, is_closed, self.color(color))])
            if mark_points:
                for p in points[start:end, :]:
                    self.add_circle(p, 2 * width, color, thickness=-1)

    def add_rectangle(self, rect, color="w", width=1):
        if not self.on:
            return
        if self.zoom != 1:
            rect = np.asarray(rect) / self.zoom
        p1 = (int(rect[0]), int(rect[1]))
        p2 = (int(rect[0] + rect[2] - 1), int(rect[1] + rect[3] - 1))
        corners = [p1, (p2[0], p1[1]), p2, (p1[0], p2[1])]
        draw_frame(self.frame, [("polyline", corners, True, self.color(color))])

    def add_circle(self, pos, radius=2, color="w", thickness=-1):
        if not self.on:
            return
        try:
            pos = (int(pos[0] / self.zoom), int(pos[1] / self.zoom))
            radius = int(math.ceil(radius / self.zoom))
        except (ValueError, OverflowError):
            return
        draw_frame(self.frame, [("circle", pos, radius, thickness < 0, self.color(color))])

    def add_points(self, points, radius=1, color="w"):
        for p in points:
            self.add_circle(p, radius, color, thickness=-1)

    def close(self):
        if self.frame is not None:
            self.out.append(self.frame)
            self.frame = None
        return np.array(self.out, np.uint8)
