"""CPU: the reference fixture (tests/golden/reference_v1.npz, written by the reference's own functions,
see tests/golden/make_golden_reference.py) -- its completeness, the CPU oracle the GPU suite trusts,
and the host-only code (regionprops, FilterCrop's rectangle, the channel picks).  No reference
checkout is read here."""
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_reference", os.path.join(ROOT, "tests", "golden", "make_golden_reference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(ROOT, "tests", "golden", "reference_v1.npz"), allow_pickle=False)


def temporal_input(ref, key):
    if key + "/input" in ref:
        return ref[key + "/input"]
    n, h, w = (int(v) for v in ref[key + "/shape"])
    v = G.frames_of(str(ref[key + "/gen"]), n, h, w, int(ref[key + "/salt"]))
    assert v.dtype.str == str(ref[key + "/dtype"])
    return v


def matches(ref, key, field, got):
    """bit for bit, dtype and shape included (by sha256 where the fixture keeps only that)"""
    got = np.asarray(got)
    if key + "/" + field in ref:
        want = ref[key + "/" + field]
        return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=True)
    return G.digest(got) == str(ref[key + "/" + field + "_sha256"])


def names(ref, group):
    return [str(n) for n in ref["names"] if str(n).startswith(group + "/")]


def test_fixture_has_every_case_and_its_shims(ref):
    assert tuple(str(s) for s in ref["shims"]) == G.SHIMS
    for group, least in (("mean", 60), ("regions", 15), ("peaks", 30), ("normalize", 30), ("crop", 15),
                         ("mono", 6), ("timediff", 1), ("regionprops", 7)):
        assert len(names(ref, group)) >= least, group
    want = {"mean/%s_n%d_7x13" % (g, n) for g in ("u8", "i16", "f32", "f64")
            for n in (1, 2, 3, 4, 31, 32, 33, 65, 300)}
    want |= {"mean/u8_hashed_40x1080x1920", "regions/two_blobs", "regions/empty", "regions/tie_equal_area",
             "regions/diagonal_contact", "regions/corners", "regions/full", "regions/row_1xN", "regions/col_Nx1",
             "peaks/u8_hashed_1080x1920", "peaks/f32_signed", "peaks/batch_3x5x7", "regionprops/line_slanted",
             "regionprops/diag_b_pos", "regionprops/antidiag_b_neg", "normalize/f32_learnt_to_f64",
             "crop/nested_three", "mono/mean4", "timediff/u8"}
    assert want <= set(str(n) for n in ref["names"])
    for w in ("u8_1x4", "u8_1x5", "u8_2x6", "u8_3x7"):                  # w % 4 in {0, 1, 2, 3}, h in {1, 2, 3}
        assert "peaks/" + w in ref["names"]


def test_issue_examples(ref):
    assert tuple(ref["regions/two_blobs/bbox"]) == (3, 2, 3, 3)
    out = dict(zip((str(k) for k in ref["regionprops_out"]), ref["regionprops/line_slanted/out"]))
    assert out["e2"] < 0 and np.isnan(out["minor_axis_length"])
    assert str(ref["regions/empty/bbox_error"]) == "IndexError"
    assert str(ref["regions/empty/largest_error"]) == "ValueError"
    # the n < 2 branch returns the last frame itself, in its own dtype, and 0
    for g, dt in (("u8", np.uint8), ("i16", np.int16), ("f32", np.float32), ("f64", np.float64)):
        key = "mean/%s_n2_7x13" % g
        assert ref[key + "/ms_mean"].dtype == dt and ref[key + "/ms_std"].shape == ()
        assert np.array_equal(ref[key + "/ms_mean"], temporal_input(ref, key)[-1])


def test_oracle_measure_mean_and_welford(ref, oracle):
    """oracle.measure_mean_numpy / measure_mean_std_numpy and the C oracle's mean / Welford updates"""
    for key in names(ref, "mean"):
        video = temporal_input(ref, key)
        assert matches(ref, key, "mean", oracle.measure_mean_numpy(video)), key
        m, s = oracle.measure_mean_std_numpy(video)
        assert matches(ref, key, "ms_mean", m) and matches(ref, key, "ms_std", s), key
        if video.dtype == np.float64:
            continue                                        # the C oracle has no float64 frames
        if video.dtype == np.uint8:
            _, cm = oracle.bg_mean_u8(video, want_diff=False)
        else:
            cm = oracle.mean_any(video)
        assert matches(ref, key, "mean", cm), key
        wm, m2 = oracle.welford_u8(video) if video.dtype == np.uint8 else oracle.welford_any(video)
        if len(video) >= 3:
            assert matches(ref, key, "ms_mean", wm) and matches(ref, key, "ms_std", np.sqrt(m2 / (len(video) - 1))), key


def test_oracle_label_stats_and_largest_region(ref, oracle):
    for key in names(ref, "regions"):
        mask = ref[key + "/mask"]
        if key + "/largest_error" in ref:
            with pytest.raises(ValueError):
                oracle.get_largest_region(mask)
            assert oracle.label(mask)[1] == 0
            continue
        region, area = oracle.get_largest_region(mask, ret_area=True)
        assert np.array_equal(region, ref[key + "/largest"]) and area == int(ref[key + "/area"]), key
        labels, count = oracle.label(mask)
        st = oracle.region_stats(labels, count)
        assert st[:, 0].sum() == int(np.count_nonzero(mask)), key
        # the reference's box is the true bounding box exactly when its rows and columns are gap-free
        x0, y0 = int(st[:, 10].min()), int(st[:, 11].min())
        x1, y1 = int(st[:, 12].max()), int(st[:, 13].max())
        assert tuple(ref[key + "/bbox"][:2]) == (x0, y0), key
        box = np.asarray(mask)[y0:y1 + 1, x0:x1 + 1] != 0
        if box.any(axis=0).all() and box.any(axis=1).all():
            assert tuple(ref[key + "/bbox"]) == (x0, y0, x1 - x0 + 1, y1 - y0 + 1), key


def test_oracle_detect_peaks(ref, oracle):
    for key in names(ref, "peaks"):
        for p in (1, 0):
            if key + "/img" in ref:
                img = ref[key + "/img"]
                got = np.stack([oracle.detect_peaks(im, bool(p)) for im in img]) if img.ndim == 3 \
                    else oracle.detect_peaks(img, bool(p))
            else:
                got = oracle.detect_peaks(G.hashed((1080, 1920), int(ref[key + "/salt"])) // 16, bool(p))
            assert matches(ref, key, "peaks_%d" % p, got), (key, p)


def test_oracle_time_difference_and_mono_mean(ref, oracle):
    f = ref["timediff/u8/frames"]
    got = np.stack([oracle.time_difference_u8(f[k + 1], f[k]) for k in range(len(f) - 1)])
    assert matches(ref, "timediff/u8", "out", got)
    assert matches(ref, "mono/mean3", "out", oracle.mono_mean_u8(ref["crop_source/col3"]))


def test_regionprops_against_the_fixture(ref):
    """host-only: the derived scalars of regionprops(moments=...), NaN axis lengths included"""
    from video.analysis.image import moments_from_spatial, regionprops
    keys = [str(k) for k in ref["regionprops_keys"]]
    for key in names(ref, "regionprops"):
        m = dict(zip(keys, (float(v) for v in ref[key + "/moments"])))
        rp = regionprops(moments=m)
        e1, e2 = rp.inertia_tensor_eigvals
        got = np.array([rp.area, rp.centroid[0], rp.centroid[1], rp.orientation, e1, e2,
                        rp.major_axis_length, rp.minor_axis_length], np.float64)
        assert np.array_equal(got, ref[key + "/out"], equal_nan=True), (key, got, ref[key + "/out"])
        # the moments the GPU path hands to regionprops are these ones
        full = moments_from_spatial(list(ref[key + "/spatial"]) + [0.0] * 4)
        assert [full[k] for k in keys] == [float(v) for v in ref[key + "/moments"]], key
    assert np.isnan(regionprops(moments=dict(zip(keys, ref["regionprops/line_slanted/moments"]))).minor_axis_length)


def _video(frames):
    """an in-memory video of any channel count (VideoMemory takes 1 or 3 only)"""
    from video.io.base import VideoBase

    class Frames(VideoBase):
        seekable = True

        def __init__(self, data):
            self.data = data
            super(Frames, self).__init__(size=(data.shape[2], data.shape[1]), frame_count=len(data),
                                         is_color=data.ndim == 4)

        def get_frame(self, index):
            return self.data[index]
    return Frames(frames)


def build_crop(ref, key, video):
    from video.filters import FilterCrop
    filt = video
    for kw in json.loads(str(ref[key + "/chain"])):
        filt = FilterCrop(filt, **kw)
    return filt


def test_filter_crop_rects_and_channel_picks(ref):
    """host-only: FilterCrop's rectangle (fractions, negatives, regions, alignment, nesting) and its
    frames, FilterMonochrome's channel picks"""
    from video.filters import FilterMonochrome
    for key in names(ref, "crop"):
        frames = ref["crop_source/" + str(ref[key + "/source"])]
        filt = build_crop(ref, key, _video(frames))
        assert filt.rect == tuple(int(v) for v in ref[key + "/rect"]), key
        got = np.stack([filt.get_frame(i) for i in range(len(frames))])
        assert matches(ref, key, "out", got), key
    for key in names(ref, "mono"):
        mode = str(ref[key + "/mode"])
        if mode == "mean":
            continue                                    # a GPU kernel: tests/test_gpu_reference.py
        frames = ref["crop_source/" + str(ref[key + "/source"])]
        filt = FilterMonochrome(_video(frames), mode)
        assert matches(ref, key, "out", np.stack([filt.get_frame(i) for i in range(len(frames))])), key
