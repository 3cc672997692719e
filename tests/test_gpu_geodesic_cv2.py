"""GPU, opportunistic: get_farthest_points' default start against REAL OpenCV -- the longest
cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) contour by cv2.arcLength(closed=True), first
point -- for the arcLength summation the library restates.  Skips cleanly without cv2."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

cv2 = pytest.importorskip("cv2", reason="OpenCV is not installed on this box")


def _cv2_p1(mask):
    res = cv2.findContours(mask.copy(), cv2.RETR_EXTERNAL, cv2.CHAIN_APPROX_SIMPLE)
    contours = res[-2]
    c = max(contours, key=lambda cnt: cv2.arcLength(cnt, closed=True))
    return int(c[0, 0, 0]), int(c[0, 0, 1])


def test_default_start_matches_cv2():
    from video import _hip, ops
    _hip.lib()
    print("\n[cv2 parity] OpenCV %s" % cv2.__version__)
    rng = np.random.default_rng(17)
    for k in range(8):
        h, w = int(rng.integers(30, 200)), int(rng.integers(30, 260))
        a = rng.random((h, w))
        for _ in range(2):
            a = (a + np.roll(a, 1, 0) + np.roll(a, 1, 1) + np.roll(a, -1, 0) + np.roll(a, -1, 1)) / 5
        m = (a > np.quantile(a, 0.55)).astype(np.uint8)
        p1 = _cv2_p1(m)
        got, _ = ops.farthest_points(m)
        ref, _ = ops.farthest_points(m, p1)
        assert tuple(got) == tuple(ref), k
