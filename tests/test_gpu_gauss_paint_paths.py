"""GPU: the matrix-core Gaussian's three outputs and the label paint at its piece boundaries, bit for bit against
the oracle (no tolerance anywhere: everything here is integer).

Gaussian (va_gauss_mfma.hip): the thresholded value is acc_min - 1 - acc, with the constant entering through the
low-byte chain of the column pass.  Constant frames pin that constant -- the taps sum to 256 and the border is
reflected, so the blur of a constant frame is the constant and the mask is all 0 / all 1 exactly at
v = thresh / thresh + 1 -- and random frames at the smallest size, at a height that is no multiple of the
32-row tile with a last strip of inactive waves, and at a partial group of eight frames run every instantiation:
bits (chain to labels; the one that runs five workgroups per CU with its Toeplitz fragments in LDS), bytes (blur
alone, blur + labels) and the byte mask.

Paint (ccl_paint_kernel, va_ccl.hip): the label image leaves in 1 KiB pieces, four pixels per lane, a piece
possibly straddling two rows.  Masks that are empty, full, or whose foreground sits at the piece, word, row and
row-block boundaries, labelled directly and through the chain, with and without statistics, under every label
source the paint pass has (the library's choice, run tables, sparse words, the large-frame mode): what any
shortcut for pieces without foreground has to keep (DESIGN.md 14 measured one and dropped it).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CLOSE5 = (("dilate", "rect", 5), ("erode", "rect", 5))


def _engine(**kw):
    from video import _hip
    from video.engine import FrameEngine
    _hip.lib()                      # loud failure without the extension / a GPU
    return FrameEngine(**kw)


# ------------------------------------------------------------------------------------------ Gaussian
def _ref_labels(oracle, mask, conn):
    labs, cnts = [], []
    for f in range(mask.shape[0]):
        lab, cnt = oracle.label(mask[f], conn)
        labs.append(lab)
        cnts.append(cnt)
    return np.stack(labs), np.array(cnts, np.int32)


def _check_three_outputs(oracle, clip, sigma, thresh, maxval=255):
    """bits, bytes and byte mask of one clip; returns the oracle's blur"""
    from video import filters as F, ops
    from video.io.memory import VideoMemory
    n, h, w = clip.shape
    blur = oracle.gaussian_u8(clip, sigma)
    mask = oracle.threshold_u8(blur, thresh, 255)
    closed = oracle.morph_u8(oracle.morph_u8(mask, oracle.DILATE, oracle.RECT, 5), oracle.ERODE, oracle.RECT, 5)
    # -- bits: the full chain to labels, nothing else requested (the flagship's instantiation)
    eng = _engine(size=(w, h), max_batch=n, sigma=sigma, thresh=thresh, morphology=CLOSE5, connectivity=4)
    assert "mfma" in eng.description
    out = eng.run(clip, want=("labels", "counts"))
    rl, rc = _ref_labels(oracle, closed, 4)
    assert np.array_equal(out["counts"], rc)
    assert np.array_equal(out["labels"], rl)
    # -- bytes + bits in one run: blur and labels (and the closed mask, unpacked from the same bits)
    out = eng.run(clip, want=("filtered", "mask", "labels", "counts"))
    eng.close()
    assert np.array_equal(out["filtered"], blur)
    assert np.array_equal(out["mask"], closed)
    assert np.array_equal(out["counts"], rc) and np.array_equal(out["labels"], rl)
    # -- bytes: FilterBlur, through the op and through the filter class
    assert np.array_equal(ops.gaussian_blur(clip, sigma), blur)
    video = F.FilterBlur(VideoMemory(clip), sigma)
    for k, frame in enumerate(video):
        assert np.array_equal(frame, blur[k]), k
    video.close()
    # -- byte mask: the chain that ends at the thresholded mask
    eng = _engine(size=(w, h), max_batch=n, sigma=sigma, thresh=thresh, maxval=maxval)
    assert "mfma" in eng.description
    eng.profile(True)
    got = eng.run(clip, want=("mask",))["mask"]
    stages = eng.stage_times()
    eng.close()
    assert "gauss_mfma_mask8" in stages
    assert np.array_equal(got, oracle.threshold_u8(blur, thresh, maxval))
    return blur


@pytest.mark.parametrize("thresh", [0, 20, 254])
@pytest.mark.parametrize("above", [0, 1])
@pytest.mark.parametrize("shape", [(2, 32, 64), (3, 97, 208)])
def test_gaussian_constant_frames_at_the_threshold(oracle, shape, thresh, above):
    """constant frames of value thresh and thresh + 1: the blur is exactly the value, the mask all 0 / all 1"""
    v = thresh + above
    clip = np.full(shape, v, np.uint8)
    blur = _check_three_outputs(oracle, clip, 5.0, thresh)
    assert (blur == v).all()
    eng = _engine(size=(shape[2], shape[1]), max_batch=shape[0], sigma=5.0, thresh=thresh, connectivity=4)
    out = eng.run(clip, want=("labels", "counts"))
    eng.close()
    assert (out["labels"] == above).all() and (out["counts"] == above).all()


@pytest.mark.parametrize("sigma", [5.0, 1.0])
@pytest.mark.parametrize("shape", [(2, 32, 64), (3, 97, 208), (9, 64, 128)])
def test_gaussian_random_frames_all_three_outputs(oracle, shape, sigma):
    rng = np.random.default_rng(shape[0] * 1000 + shape[2] + int(sigma))
    clip = rng.integers(0, 256, shape, dtype=np.uint8)
    clip[0, :9, :] = 255                       # saturated and empty regions next to the borders
    clip[-1, :, -20:] = 0
    blur = _check_three_outputs(oracle, clip, sigma, 127, maxval=200)
    frac = (blur > 127).mean()
    assert 0.05 < frac < 0.95                  # a mask of both values, so that the labels say something


# --------------------------------------------------------------------------------------------- paint
PAINT_SHAPES = [(2, 8, 208),      # pieces straddle rows
                (1, 12, 1920),
                (1, 10, 208),     # height no multiple of 4: the per-chunk path
                (1, 8, 210),      # no vector stores
                (1, 8, 2112)]     # the wide form (rows of 66 mask words)
# label sources of the paint pass (va_test_hook_labelling): the library's choice, the per-frame kernel's run
# tables, sparse words in the label image, the per-frame kernel's large-frame mode (a tiny run-table cap)
PAINT_MODES = {"default": (0, 0), "run-table": (2, 0), "sparse": (3, 0), "large-frame": (2, 7)}


def _paint_masks(shape):
    """name -> (n, h, w) uint8 mask; frame f is frame 0 rolled down by f rows, so that frames differ"""
    n, h, w = shape
    base = {}
    base["zeros"] = np.zeros((h, w), np.uint8)
    base["ones"] = np.ones((h, w), np.uint8)
    every = np.zeros((h, w), np.uint8)
    for y in (0, 3, 4, h - 1):
        for x in (0, 255, 256, w - 1):
            if x < w:
                m = np.zeros((h, w), np.uint8)
                m[y, x] = 1
                base["pixel_y%d_x%d" % (y, x)] = m
                every[y, x] = 1
    base["pixels_together"] = every
    run = np.zeros((h, w), np.uint8)
    run[1, 250:261] = 1                        # (clipped to the row where the frame is narrower)
    run[h - 1, 250:261] = 1
    base["run_250_260"] = run
    wrap = np.zeros((h, w), np.uint8)
    for y in (1, 3):                           # inside a block of four rows, and from one block into the next
        wrap[y, w - 5:] = 1
        wrap[y + 1, :5] = 1
    base["run_row_end_to_row_start"] = wrap
    return {k: np.stack([np.roll(m, f, axis=0) for f in range(n)]) for k, m in base.items()}


_paint_refs = {}


def _paint_cases(oracle, shape):
    """[(name, masks, {conn: (labels, counts, [stats per frame])})], computed once per shape"""
    if shape not in _paint_refs:
        cases = []
        for name, masks in _paint_masks(shape).items():
            ref = {}
            for conn in (4, 8):
                rl, rc = _ref_labels(oracle, masks, conn)
                rs = [oracle.region_stats(rl[f], int(rc[f])) for f in range(shape[0])]
                ref[conn] = (rl, rc, rs)
            cases.append((name, masks, ref))
        _paint_refs[shape] = cases
    return _paint_refs[shape]


@pytest.fixture(params=sorted(PAINT_MODES))
def paint_mode(request):
    from video import _hip
    path, lds_runs = PAINT_MODES[request.param]
    _hip.check(_hip.lib().va_test_hook_labelling(path, lds_runs))
    yield request.param
    _hip.check(_hip.lib().va_test_hook_labelling(0, 0))


@pytest.mark.parametrize("shape", PAINT_SHAPES)
def test_paint_background_pieces_and_boundaries(oracle, shape, paint_mode):
    from video import ops
    n, h, w = shape
    ml = 32
    cases = _paint_cases(oracle, shape)
    for conn in (4, 8):
        eng = _engine(size=(w, h), max_batch=n, thresh=0, connectivity=conn, max_labels=ml)
        for name, masks, ref in cases:
            rl, rc, rs = ref[conn]
            where = (name, conn, paint_mode)
            # -- labelled directly
            lab, cnt = ops.label(masks, conn)
            assert np.array_equal(cnt, rc), where
            assert np.array_equal(lab, rl), where
            # -- through the chain (threshold at 0 gives the mask back), without and with statistics
            frames = masks * np.uint8(255)
            out = eng.run(frames, want=("labels", "counts"))
            assert np.array_equal(out["counts"], rc), where
            assert np.array_equal(out["labels"], rl), where
            out = eng.run(frames, want=("labels", "counts", "stats"))
            assert np.array_equal(out["counts"], rc), where
            assert np.array_equal(out["labels"], rl), where
            for f in range(n):
                k = min(int(rc[f]), ml)
                assert np.array_equal(out["stats"][f, :k, :14], rs[f][:k, :14]), where + (f,)
        eng.close()
