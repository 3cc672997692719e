"""GPU, and only where cv2 is installed: the best position of ops.match_templates equals cv2.minMaxLoc's on
cv2.matchTemplate for all six methods, on inputs whose best exceeds the runner-up by a clear planted margin (so that
cv2's float32 and DFT rounding cannot reorder them).  The largest deviation of the float64 maps from cv2's float32
maps is printed, not asserted: nobody has measured it ("Template matching")."""
import numpy as np
import pytest

import template_match_checks as K

cv2 = pytest.importorskip("cv2")

pytestmark = pytest.mark.gpu


def test_best_positions_equal_cv2_min_max_loc():
    from video.analysis import image
    rng = np.random.default_rng(53)
    scene = rng.integers(60, 120, (90, 130)).astype(np.uint8)
    template = rng.integers(0, 256, (13, 18), dtype=np.uint8)
    template[:4, :5] = 255                              # bright enough that plain correlation peaks on the copy too
    scene[41:54, 77:95] = template
    for code, method in enumerate(K.METHODS):           # cv2.TM_SQDIFF .. cv2.TM_CCOEFF_NORMED are 0 .. 5
        theirs = cv2.matchTemplate(scene, template, code)
        lo, hi, lo_at, hi_at = cv2.minMaxLoc(theirs)
        want = lo_at if method.startswith("sqdiff") else hi_at
        position, score = image.find_template(scene, template, method=method)
        ours = image.match_template(scene, template, method=method)
        print(method, "largest deviation from cv2's float32 map:", float(np.abs(ours - theirs).max()),
              "at scores up to", float(np.abs(ours).max()))
        assert position == tuple(want) == (77, 41), method
