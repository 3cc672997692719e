"""CPU: the pinned 8-bit affine warp ("Affine warps and line scans") -- the fixture line_scan_v1.npz is
complete and reproduced by the NumPy restatement of tests/golden/make_golden_line_scan.py, the restatement has the
properties the definition promises, ops.affine_transforms is the same arithmetic, and the host-side functions of
video.analysis.image follow the fixture.  Reads the npz and the generator's restatement only."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_line_scan", os.path.join(ROOT, "tests", "golden", "make_golden_line_scan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(ROOT, "tests", "golden", "line_scan_v1.npz"), allow_pickle=False)


def test_fixture_is_complete_and_reproduced(fx):
    imgs = G.images()
    want = {"shims"} | {"image/%s" % n for n in imgs} | {"profile/%s" % n for n in G.profiles()}
    want |= {"scan/%d/%s" % (k, f) for k in range(len(G.SCAN_CASES))
             for f in ("points", "half_width", "matrix", "strip", "profile")}
    want |= {"sub/%d/%s" % (k, f) for k in range(len(G.SUBIMAGE_CASES)) for f in ("matrix", "image")}
    want |= {"steepest/%d" % k for k in range(len(G.STEEPEST_CASES))}
    assert set(fx.files) == want
    assert fx["shims"].tolist() == G.SHIMS
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "line_scan_v1.npz")) < 400 * 1024
    for name, img in imgs.items():
        assert np.array_equal(fx["image/%s" % name], img), name
    for k, (name, p1, p2, hw) in enumerate(G.SCAN_CASES):
        M, strip = G.line_scan_strip(imgs[name], p1, p2, hw)
        assert np.array_equal(fx["scan/%d/points" % k], np.array([p1, p2], np.float64)) and fx["scan/%d/half_width" % k] == hw
        assert np.array_equal(fx["scan/%d/matrix" % k], M), k
        assert fx["scan/%d/strip" % k].dtype == np.uint8 and np.array_equal(fx["scan/%d/strip" % k], strip), k
        prof = fx["scan/%d/profile" % k]
        assert prof.dtype == np.float64 and np.array_equal(prof, G.line_scan(imgs[name], p1, p2, hw)), k
        assert np.array_equal(prof, strip.mean(axis=0)), k
    for k, (name, sx, sy, width, height) in enumerate(G.SUBIMAGE_CASES):
        src, dst, dsize = G.subimage_geometry(sx, sy, width, height)
        assert np.array_equal(fx["sub/%d/matrix" % k], G.get_affine_transform(src, dst)), k
        sub = fx["sub/%d/image" % k]
        assert sub.dtype == np.uint8 and sub.shape == (dsize[1], dsize[0]), k
        assert np.array_equal(sub, G.get_subimage(imgs[name], sx, sy, width, height)), k
    for name, p in G.profiles().items():
        assert np.array_equal(fx["profile/%s" % name], p), name
    # the cases cover what they are there for
    assert any(fx["scan/%d/strip" % k].max() == 0 for k in range(len(G.SCAN_CASES)))            # wholly outside
    assert any(fx["scan/%d/strip" % k].min() == 255 for k in range(len(G.SCAN_CASES)))          # the top of the range
    assert {fx["scan/%d/strip" % k].shape[0] for k in range(len(G.SCAN_CASES))} >= {1, 2, 3, 5, 10, 14}


def test_identity_and_axis_aligned_scans_are_exact():
    img = G.images()["noise"]
    assert img.shape == (60, 80)
    ident = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    assert np.array_equal(G.warp_affine(img, ident, (80, 60)), img)
    assert np.array_equal(G.warp_affine(img, ident, (80, 60), inverse=True), img)
    # one pixel further on either axis: the constant border
    big = G.warp_affine(img, ident, (82, 61))
    assert np.array_equal(big[:60, :80], img) and not big[60:].any() and not big[:, 80:].any()
    strip = G.line_scan_strip(img, (10, 30), (50, 30), 3)[1]
    assert np.array_equal(strip, img[27:33, 10:50])
    assert np.array_equal(G.line_scan(img, (10, 30), (50, 30), 3), img[27:33, 10:50].mean(axis=0))
    strip = G.line_scan_strip(img, (10, 30), (10, 5), 2)[1]
    assert np.array_equal(strip, img[30:5:-1, 8:12].T)
    # a translation by half a pixel is the rounded mean of two neighbours
    half = G.warp_affine(img, np.array([[1.0, 0.0, -0.5], [0.0, 1.0, 0.0]]), (79, 60))
    assert np.array_equal(half, (img[:, :79].astype(int) + img[:, 1:] + 1) >> 1)


def test_inverse_flag_takes_the_inverted_matrix():
    img = G.images()["ramp"]
    for k, (name, p1, p2, hw) in enumerate(G.SCAN_CASES[:10]):
        src, dst, rows, cols = G.scan_geometry(p1, p2, hw)
        M = G.get_affine_transform(src, dst)
        assert np.array_equal(G.warp_affine(img, G.invert(M), (cols, rows), inverse=True),
                              G.warp_affine(img, M, (cols, rows))), k
    assert np.array_equal(G.invert(np.zeros((2, 3))), np.zeros((2, 3)))          # D == 0: the zero map, as OpenCV


def test_table_form_equals_the_short_formula():
    """OpenCV multiplies by a table of 15-bit weights; the table's one saturated entry cannot change a result"""
    for spill in (1, 2, 3):
        tab = G.bilinear_table(spill)
        assert tab[0, 0].tolist().count(32767) == 1 and tab[0, 0].sum() == 32768
        fy, fx = np.mgrid[:32, :32]
        exact = np.stack([(32 - fx) * (32 - fy), fx * (32 - fy), (32 - fx) * fy, fx * fy], -1) * 32
        exact[0, 0] = tab[0, 0]
        assert np.array_equal(tab, exact)
    rng = np.random.default_rng(21)
    imgs = [G.images()["noise"], G.images()["white"], rng.integers(0, 2, (60, 80), dtype=np.uint8) * np.uint8(255)]
    for k in range(120):
        img = imgs[k % 3]
        p1, p2 = rng.uniform(-10, 85, 2), rng.uniform(-10, 85, 2)
        if k % 4 == 0:
            p1, p2 = np.rint(p1), np.rint(p2) + 1
        hw = float(rng.choice(G.GPU_HALF_WIDTHS))
        src, dst, rows, cols = G.scan_geometry(p1, p2, hw)
        if cols < 1:
            continue
        M = G.get_affine_transform(src, dst)
        assert np.array_equal(G.warp_affine_table(img, M, (cols, rows), spill=1 + k % 3),
                              G.warp_affine(img, M, (cols, rows))), k


def test_affine_transforms_is_the_restatements_arithmetic():
    from video import ops
    src, dst = G.random_triples(31, 400)
    got = ops.affine_transforms(src, dst)
    assert got.shape == (400, 2, 3) and got.dtype == np.float64
    for k in range(400):
        assert np.array_equal(got[k], G.get_affine_transform(src[k], dst[k])), k
    # the points really are mapped (to float32 accuracy of the inputs)
    s32, d32 = src.astype(np.float32).astype(np.float64), dst.astype(np.float32).astype(np.float64)
    mapped = np.einsum("kij,kpj->kpi", got[:, :, :2], s32) + got[:, None, :, 2]
    assert np.max(np.abs(mapped - d32)) < 1e-6
    one = ops.affine_transforms(src[7], dst[7])
    assert one.shape == (1, 2, 3) and np.array_equal(one[0], got[7])
    assert ops.affine_transforms(np.zeros((0, 3, 2)), np.zeros((0, 3, 2))).shape == (0, 2, 3)
    line = np.array([[0, 0], [1, 1], [2, 2]], np.float64)
    with pytest.raises(ValueError):
        G.get_affine_transform(line, dst[0])
    with pytest.raises(ValueError, match="item 3"):
        bad = src[:5].copy()
        bad[3] = line
        ops.affine_transforms(bad, dst[:5])


def test_line_scan_tables_equal_the_restatement():
    from video import ops
    batch = G.gpu_batch()
    p1 = np.array([b[1] for b in batch], np.float64)
    p2 = np.array([b[2] for b in batch], np.float64)
    hw = np.array([b[3] for b in batch], np.float64)
    mats, rows, cols = ops.line_scan_tables(p1, p2, hw)
    for k, (f, a, b, w) in enumerate(batch):
        src, dst, r, c = G.scan_geometry(a, b, w)
        assert (rows[k], cols[k]) == (r, c), k
        assert np.array_equal(mats[k], G.get_affine_transform(src, dst)), k
    assert set(G.GPU_LENGTHS) <= set(cols.tolist())
    assert {int(2 * w) for w in G.GPU_HALF_WIDTHS} <= set(rows.tolist())


def test_get_steepest_point_follows_the_fixture(fx):
    from video.analysis.image import get_steepest_point
    for k, (name, direction, smoothing) in enumerate(G.STEEPEST_CASES):
        got = get_steepest_point(fx["profile/%s" % name], direction, smoothing)
        want = float(fx["steepest/%d" % k])
        assert (np.isnan(got) and np.isnan(want)) or got == want, (k, got, want)
    assert get_steepest_point(fx["profile/step"], 1) == 37.5 and get_steepest_point(fx["profile/step"], -1) == 12.5
    assert np.isnan(get_steepest_point([1.0])) and np.isnan(get_steepest_point([]))


def test_python2_round():
    from video.analysis import image
    for x, want in ((0.5, 1), (1.5, 2), (2.5, 3), (-0.5, -1), (-2.5, -3), (2.4999, 2), (7.0, 7), (0.49999999999999994, 0)):
        assert image._round_half_away(x) == want and G.py2_round(x) == want, x


def test_argument_checks():
    """everything that is refused on the host is refused before the GPU is touched"""
    from video import ops
    from video.analysis import image
    img = G.images()["noise"]
    for bad in (img.astype(np.float32), img.astype(np.int16), np.zeros((4, 5, 3), np.uint8)):
        with pytest.raises(TypeError, match="uint8"):
            image.line_scan(bad, (1, 1), (3, 3))
        with pytest.raises(TypeError, match="uint8"):
            image.get_subimage(bad, (0, 4), (0, 4))
    with pytest.raises(TypeError, match="uint8"):
        image.line_scans(img.astype(np.float64), [(1, 1)], [(3, 3)])
    with pytest.raises(TypeError, match="uint8"):
        ops.warp_affine(img.astype(np.float32), np.zeros((1, 2, 3)), [(3, 3)])
    with pytest.raises(ValueError, match="empty"):
        image.line_scan(img, (5, 5), (5.5, 5.5))                     # int(length) == 0
    with pytest.raises(ValueError, match="empty"):
        image.line_scan(img, (5, 5), (25, 5), half_width=0.4)        # int(2 hw) == 0
    with pytest.raises(ValueError, match="empty"):
        image.line_scan(img, (5, 5), (5, 5))
    with pytest.raises(ValueError, match="empty"):
        image.get_subimage(img, (5, 25), (5, 25), width=0.4)
    with pytest.raises(ValueError):
        image.get_subimage(img, (5, 5), (5, 25))                     # an empty slice
    with pytest.raises(ValueError, match="collinear"):
        image.get_subimage(img, (5, 25), (5, 5), width=10, height=10)
    with pytest.raises(ValueError, match="exceeds"):
        ops.line_scans(img, [(0, 0)], [(40000, 0)])
    with pytest.raises(ValueError, match="frame_index"):
        ops.line_scans(np.stack([img, img]), [(0, 0)], [(10, 0)])
    with pytest.raises(ValueError, match="frame_index"):
        ops.line_scans(np.stack([img, img]), [(0, 0)], [(10, 0)], frame_index=[2])
    with pytest.raises(ValueError):
        ops.line_scans(img, [(0, 0), (1, 1)], [(10, 0)])
    with pytest.raises(ValueError):
        ops.line_scans(img, [(0, 0)], [(10, 0)], half_width=[1, 2])
    with pytest.raises(ValueError, match="finite"):
        ops.line_scans(img, [(0, 0)], [(np.nan, 0)])
    with pytest.raises(ValueError, match="empty"):
        ops.warp_affine(img, np.zeros((1, 2, 3)), [(0, 3)])
    with pytest.raises(ValueError, match="limited"):
        ops.warp_affine(img, np.zeros((1, 2, 3)), [(3, 40000)])
    with pytest.raises(ValueError):
        ops.warp_affine(img, np.zeros((2, 2, 3)), [(3, 3)])
    with pytest.raises(ValueError):
        image.line_scans(np.stack([img, img]), [[(0, 0)]], [[(5, 0)]])
    with pytest.raises(ValueError, match="limits"):
        G.warp_affine(img, np.array([[1e-7, 0, 0], [0, 1.0, 0]]), (50, 5))   # the inverse leaves int32
    with pytest.raises(ValueError, match="limits"):
        G.warp_affine(img, np.eye(2, 3), (40000, 5))
    assert ops.line_scans(img, np.zeros((0, 2)), np.zeros((0, 2))) == []
    assert ops.warp_affine(img, np.zeros((0, 2, 3)), np.zeros((0, 2))) == []
    assert image.line_scans(np.stack([img, img]), [[], []], [[], []]) == [[], []]
