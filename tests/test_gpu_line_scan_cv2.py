"""GPU vs a real cv2, where one is installed: cv2.getAffineTransform and cv2.warpAffine (INTER_LINEAR,
BORDER_CONSTANT 0) on the cases of test_gpu_line_scan.py.  The pinned definition is the classical fixed-point path
of OpenCV 2.4 .. 4.10; OpenCV 4.11 and later warp with float kernels and may differ by one grey level, which this
file would then show.  Skips cleanly without cv2."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
cv2 = pytest.importorskip("cv2", reason="OpenCV is not installed on this box")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_line_scan", os.path.join(ROOT, "tests", "golden", "make_golden_line_scan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()


def test_matrices_match_cv2():
    from video import ops
    print("\n[cv2 parity] OpenCV %s" % cv2.__version__)
    src, dst = G.random_triples(31, 400)
    got = ops.affine_transforms(src, dst)
    for k in range(len(src)):
        want = cv2.getAffineTransform(src[k].astype(np.float32), dst[k].astype(np.float32))
        assert np.array_equal(got[k], want), k


def test_line_scans_match_cv2():
    from video import ops
    frames, cases = G.gpu_frames(), G.gpu_batch()
    got = ops.line_scans(frames, [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases],
                         frame_index=[c[0] for c in cases])
    for k, (f, p1, p2, hw) in enumerate(cases):
        s, d, rows, cols = G.scan_geometry(p1, p2, hw)
        strip = cv2.warpAffine(frames[f], cv2.getAffineTransform(s, d), (cols, rows))
        assert np.array_equal(got[k], strip.mean(axis=0)), k


def test_subimages_and_warps_match_cv2():
    from video import ops
    from video.analysis import image
    imgs = G.images()
    for k, (name, sx, sy, width, height) in enumerate(G.SUBIMAGE_CASES):
        s, d, dsize = G.subimage_geometry(sx, sy, width, height)
        want = cv2.warpAffine(imgs[name], cv2.getAffineTransform(s, d), dsize)
        assert np.array_equal(image.get_subimage(imgs[name], sx, sy, width, height), want), k
    frame = np.random.default_rng(42).integers(0, 256, (240, 323), dtype=np.uint8)
    c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
    M = np.array([[c, s, 80.0], [-s, c, 120.0]])
    assert np.array_equal(ops.warp_affine(frame, M, [(300, 500)])[0], cv2.warpAffine(frame, M, (500, 300)))
    assert np.array_equal(ops.warp_affine(frame, M, [(300, 500)], inverse=True)[0],
                          cv2.warpAffine(frame, M, (500, 300), flags=cv2.INTER_LINEAR | cv2.WARP_INVERSE_MAP))
