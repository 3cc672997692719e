"""GPU: the per-frame labelling kernel's list of non-empty spans (ccl_frame_kernel, va_ccl.hip), bit for bit
against the oracle (labels and counts are integers: no tolerance anywhere).

In its direct form (rows of at most 64 mask words, 16-byte aligned) the kernel's first sweep appends the index
of every (row, 256-pixel span) that holds foreground to a list in LDS, and the link phase visits the listed
spans only, loading the span, the row above it and the words on either side from global memory; frames whose
list is long take the dense sweep over every span instead.  The shapes are the smallest at which that can go
wrong -- half a span, one span across the 8-row boundary of a wave, a last group of 4 words with rows across
the 128-row boundary of a sweep step, all eight groups full, three sweep steps, and a frame wider than 2048
pixels, which the kernel sweeps 4 rows per wave with 16 lanes per row -- and the masks put contacts
exactly where the list form reads differently from the sweep: across the span boundary at x = 255 / 256
(vertical and both diagonals), across rows 7/8 and 127/128, with empty and full lists, long union chains and
late merges.  Every mask runs under four label sources of va_test_hook_labelling: the list (path 2), the dense
sweep forced (path 5), the staged form (path 4) and the large-frame mode (path 2 with a tiny run table).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(2, 7, 128),       # w32 = 4: half a span, one group
          (2, 9, 256),       # one full span; rows cross the 8-row wave boundary
          (3, 130, 1920),    # the last group has 4 words; rows 127/128 cross a sweep step
          (2, 129, 2048),    # all 8 groups full
          (1, 257, 640),     # three sweep steps
          (2, 9, 2304)]      # wider than 2048: 4 rows per wave, 16 lanes per row (9 of them with words)
MODES = {"list": (2, 0), "dense": (5, 0), "staged": (4, 0), "large-frame": (2, 7)}


def _discs(h, w, seed, target=0.08):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    m = np.zeros((h, w), np.uint8)
    rmax = max(2, min(h, w) // 4)
    for _ in range(400):
        if m.mean() >= target:
            break
        r = int(rng.integers(1, rmax + 1))
        cy, cx = int(rng.integers(0, h)), int(rng.integers(0, w))
        m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1
    return m


def _spiral(h, w, pitch=4):
    """a one-pixel rectangular spiral, arms `pitch` apart: one component, found through late merges"""
    m = np.zeros((h, w), np.uint8)
    top, left, bottom, right = 0, 0, h - 1, w - 1
    first = True
    while top <= bottom and left <= right:
        m[top, (left if first else max(left - pitch, 0)):right + 1] = 1
        m[top:bottom + 1, right] = 1
        if bottom - top >= pitch and right - left >= pitch:
            m[bottom, left:right + 1] = 1
            m[top + pitch:bottom + 1, left] = 1
        first = False
        top, left, bottom, right = top + pitch, left + pitch, bottom - pitch, right - pitch
    return m


def _masks(shape):
    """name -> (n, h, w) uint8 mask; frame f is frame 0 rolled down by f rows, so that frames differ"""
    n, h, w = shape
    z = lambda: np.zeros((h, w), np.uint8)
    base = {"zeros": z(), "ones": np.ones((h, w), np.uint8)}
    corners = z()
    for y in (0, h - 1):
        for x in (0, w - 1):
            m = z()
            m[y, x] = 1
            base["pixel_y%d_x%d" % (y, x)] = m
            corners[y, x] = 1
    base["corners"] = corners
    if w > 256:
        for x in (255, 256):
            m = z()
            m[h // 2, x] = 1
            base["pixel_x%d" % x] = m
    # the three contacts between a row and the row above it, placed at the span boundary (x = 255 / 256)
    # for every row pair of interest, and at an ordinary column across the wave / sweep-step row boundaries
    xs = [w // 2 - 1] + ([255] if w > 256 else [])          # xl: the pair of columns is (xl, xl + 1)
    ys = sorted({1, h - 1} | {y for y in (8, 128) if y < h})
    for xl in xs:
        for y in ys:
            tag = "_x%d_y%d" % (xl, y)
            m = z()
            m[y, xl + 1] = m[y - 1, xl + 1] = 1
            base["vertical" + tag] = m
            m = z()
            m[y, xl + 1] = m[y - 1, xl] = 1                 # (y, 256) with (y - 1, 255)
            base["diag_down_right" + tag] = m
            m = z()
            m[y, xl] = m[y - 1, xl + 1] = 1                 # (y, 255) with (y - 1, 256)
            base["diag_down_left" + tag] = m
    # a comb: teeth every 3 columns, joined only by the last row; few enough teeth for the LDS run table
    x0 = 240 if w > 300 else 0
    teeth = max(2, min((w - x0 + 2) // 3, 6000 // h))
    comb = z()
    comb[:h - 1, x0:x0 + 3 * teeth:3] = 1
    comb[h - 1, x0:x0 + 3 * (teeth - 1) + 1] = 1
    base["comb"] = comb
    base["comb_upside_down"] = comb[::-1].copy()
    base["spiral"] = _spiral(h, w)
    base["discs"] = _discs(h, w, seed=h * 7 + w)
    yy, xx = np.mgrid[:h, :w]
    base["checkerboard_2x2"] = (((yy >> 1) + (xx >> 1)) & 1).astype(np.uint8)
    return {k: np.stack([np.roll(m, f, axis=0) for f in range(n)]) for k, m in base.items()}


_refs = {}


def _cases(oracle, shape):
    """[(name, masks, {conn: (labels, counts)})], computed once per shape and left unchanged"""
    if shape not in _refs:
        cases = []
        for name, masks in _masks(shape).items():
            ref = {conn: oracle.label_batch(masks, conn) for conn in (4, 8)}
            cases.append((name, masks, ref))
        _refs[shape] = cases
    return _refs[shape]


@pytest.fixture(params=sorted(MODES))
def label_mode(request):
    from video import _hip
    path, lds_runs = MODES[request.param]
    _hip.check(_hip.lib().va_test_hook_labelling(path, lds_runs))
    yield request.param
    _hip.check(_hip.lib().va_test_hook_labelling(0, 0))


def test_masks_are_what_they_claim(oracle):
    """frame 0 (later frames are rolled, which may cut a contact at the frame's edge): the diagonal contacts join
    under 8-connectivity and stay apart under 4, the vertical ones, the combs and the spiral are one component"""
    for shape in SHAPES:
        for name, masks, ref in _cases(oracle, shape):
            c4, c8 = int(ref[4][1][0]), int(ref[8][1][0])
            if name.startswith("diag_"):
                assert (c4, c8) == (2, 1), (shape, name)
            elif name.startswith("vertical") or name.startswith("comb") or name == "spiral":
                assert (c4, c8) == (1, 1), (shape, name)
        d = _masks(shape)["discs"]
        assert 0.04 < d.mean() < 0.16, shape


@pytest.mark.parametrize("shape", SHAPES)
def test_labels_equal_the_oracle(oracle, shape, label_mode):
    from video import ops
    for name, masks, ref in _cases(oracle, shape):
        for conn in (4, 8):
            rl, rc = ref[conn]
            lab, cnt = ops.label(masks, conn)
            assert np.array_equal(cnt, rc), (name, conn, label_mode)
            assert np.array_equal(lab, rl), (name, conn, label_mode)


@pytest.mark.parametrize("shape", [(3, 130, 1920), (1, 257, 640)])
def test_list_order_does_not_show(oracle, shape):
    """the order of the span list differs from run to run; labels and counts must not"""
    from video import _hip, ops
    masks = _masks(shape)["discs"]
    _hip.check(_hip.lib().va_test_hook_labelling(2, 0))
    try:
        for conn in (4, 8):
            lab1, cnt1 = ops.label(masks, conn)
            lab2, cnt2 = ops.label(masks, conn)
            assert np.array_equal(cnt1, cnt2) and np.array_equal(lab1, lab2), conn
            rl, rc = oracle.label_batch(masks, conn)
            assert np.array_equal(cnt1, rc) and np.array_equal(lab1, rl), conn
    finally:
        _hip.check(_hip.lib().va_test_hook_labelling(0, 0))
