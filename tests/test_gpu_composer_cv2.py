"""GPU vs a real cv2, where one is installed: cv2.polylines, drawContours, rectangle, circle, add and addWeighted on
the drawing and blend cases of test_gpu_composer.py.  Skips cleanly without cv2.  This file has not run anywhere
yet (no environment of the project has OpenCV): DESIGN.md §9, "Composer", says what is expected and unverified."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
cv2 = pytest.importorskip("cv2", reason="OpenCV is not installed on this box")

import test_gpu_composer as T  # noqa: E402

H, W = T.H, T.W


def _cv_color(color):
    return tuple(int(v) for v in np.atleast_1d(color))


def _cv_draw(frame, commands):
    frame = np.ascontiguousarray(frame)
    for cmd in commands:
        if cmd[0] == "polyline":
            pts = np.asarray(cmd[1], np.int32).reshape(-1, 1, 2)
            if len(pts):
                cv2.polylines(frame, [pts], bool(cmd[2]), _cv_color(cmd[3]), 1)
        else:
            cv2.circle(frame, tuple(int(v) for v in cmd[1]), int(cmd[2]), _cv_color(cmd[4]), -1 if cmd[3] else 1)
    return frame


@pytest.mark.parametrize("c", (1, 3), ids=("mono", "rgb"))
def test_drawing_matches_cv2(c):
    from video import ops
    print("\n[cv2 parity] OpenCV %s" % cv2.__version__)
    cases = T._draw_cases(c)
    for name in ("tiny",):                       # cv2 rejects an empty polyline; the one-point cases stay
        cases[name] = [cmd for cmd in cases[name] if len(cmd[1])]
    cases["circles"] = [cmd for cmd in cases["circles"] if cmd[2] >= 0]          # cv2 asserts radius >= 0
    frames = T._frames(T._rng("frames", c, H), len(cases), H, W, c)
    got = ops.draw(frames, list(cases.values()))
    for i, (name, commands) in enumerate(cases.items()):
        assert np.array_equal(got[i], _cv_draw(frames[i].copy(), commands)), name


def test_contours_and_rectangle_match_cv2():
    from video import ops
    yy, xx = np.mgrid[:H, :W]
    mask = (((xx - 20) ** 2 + (yy - 15) ** 2 < 90) | ((xx - 40) ** 2 + (yy - 28) ** 2 < 50)).astype(np.uint8)
    frame = T._frames(T._rng("cv2"), 1, H, W, 3)
    contours = ops.find_contours(mask)
    p1, p2 = (4, 30), (47, 6)
    rect = [p1, (p2[0], p1[1]), p2, (p1[0], p2[1])]
    got = ops.draw(frame, [[("polyline", c, True, (255, 0, 9)) for c in contours] + [("polyline", rect, True, (1, 2, 3))]])
    want = frame[0].copy()
    cv2.drawContours(want, contours, -1, (255, 0, 9), 1)
    cv2.rectangle(want, p1, p2, (1, 2, 3), 1)
    assert np.array_equal(got[0], want)


@pytest.mark.parametrize("weight", (0.0, 1.0, 0.5, 0.3))
def test_add_and_blend_match_cv2(weight):
    from video import ops
    v, u = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    got = ops.compose_layers(v[None], [[("blend", u, weight, None)]])[0]
    assert np.array_equal(got, cv2.addWeighted(v, 1 - weight, u, weight, 0))
    mask = (v > u).astype(np.uint8)
    got = ops.compose_layers(v[None], [[("add", u, mask)]])[0]
    assert np.array_equal(got, cv2.add(v, u, v.copy(), mask=mask))
