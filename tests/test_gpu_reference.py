"""GPU: the package's public functions and filters against results of the reference's OWN functions
(tests/golden/reference_v1.npz, see tests/golden/make_golden_reference.py), bit for bit, dtype and
shape included.  Every comparison is exact: the kernels restate NumPy's operation order and types
(float64 running mean / Welford with -ffp-contract=off, float32 arithmetic for float32 frames in
FilterNormalize), so no tolerance is needed anywhere."""
import numpy as np
import pytest

from test_reference_golden_host import G, _video, build_crop, matches, names, ref, temporal_input  # noqa: F401

pytestmark = pytest.mark.gpu


def test_measure_mean_and_std(ref):
    """measure_mean / measure_mean_std: uint8 (bg_mean_u8, welford_u8), int16 / float32 / float64
    (temporal_stats<T>), 1 .. 300 frames, the n < 2 branch, constant and alternating videos, and one
    40 x 1080 x 1920 video"""
    from video.analysis.video import measure_mean, measure_mean_std
    for key in names(ref, "mean"):
        video = temporal_input(ref, key)
        assert matches(ref, key, "mean", measure_mean(video)), key
        m, s = measure_mean_std(video)
        assert matches(ref, key, "ms_mean", m), key
        assert matches(ref, key, "ms_std", s), key


def test_measure_mean_batch_split(ref):
    """the batch size a video is fed in does not change a bit"""
    from video.analysis.video import measure_mean, measure_mean_std
    for key in ("mean/u8_n65_7x13", "mean/i16_n65_7x13", "mean/f32_n65_7x13", "mean/f64_n65_7x13",
                "mean/f32_n33_17x64"):
        video = temporal_input(ref, key)
        for b in (1, 7, 32):
            assert matches(ref, key, "mean", measure_mean(video, batch=b)), (key, b)
            m, s = measure_mean_std(video, batch=b)
            assert matches(ref, key, "ms_mean", m) and matches(ref, key, "ms_std", s), (key, b)


def test_float64_frames_from_filter_normalize(ref):
    """FilterNormalize(dtype=np.float64) emits float64 frames; measure_mean takes them"""
    from video.analysis.video import measure_mean, measure_mean_std
    from video.filters import FilterNormalize
    from video.io.memory import VideoMemory
    key = "normalize/u8_learnt_to_f64"
    frames = np.stack(list(FilterNormalize(VideoMemory(ref[key + "/frames"]), dtype=np.float64)))
    assert matches(ref, key, "out", frames)
    mean = measure_mean(frames)
    m, s = measure_mean_std(frames)
    # the reference's update in NumPy's own float64 arithmetic (the lifted function's results for
    # float64 videos are the mean/f64_* cases of test_measure_mean_and_std)
    r, q, w = np.zeros(frames.shape[1:]), np.zeros(frames.shape[1:]), np.zeros(frames.shape[1:])
    for n, f in enumerate(frames):
        r = r * n / (n + 1) + f / (n + 1)
        delta = f - q
        q = q + delta / (n + 1)
        w = w + delta * (f - q)
    assert mean.dtype == np.float64 and np.array_equal(mean, r)
    assert np.array_equal(m, q) and np.array_equal(s, np.sqrt(w / (len(frames) - 1)))
    with pytest.raises(TypeError):
        measure_mean(frames.astype(np.float16))


def test_largest_region_and_bounding_box(ref):
    from video.analysis.regions import find_bounding_box, get_largest_region
    for key in names(ref, "regions"):
        mask = ref[key + "/mask"]
        if key + "/bbox_error" in ref:
            with pytest.raises(IndexError):
                find_bounding_box(mask)
        else:
            assert find_bounding_box(mask) == tuple(int(v) for v in ref[key + "/bbox"]), key
        if key + "/largest_error" in ref:
            with pytest.raises(ValueError):
                get_largest_region(mask)
            continue
        region, area = get_largest_region(mask, ret_area=True)
        assert matches(ref, key, "largest", region) and area == int(ref[key + "/area"]), key
        assert np.array_equal(get_largest_region(mask), region), key
    assert find_bounding_box(ref["regions/two_blobs/mask"]) == (3, 2, 3, 3)


def test_detect_peaks(ref):
    """detect_peaks_kernel<u8, f32> and detect_peaks_u8x4_kernel: every w % 4, h in 1..3, plateaus,
    zero background at the border, -0.0 and infinities, batches whose frames straddle quads"""
    from video import _hip, ops
    from video.analysis.image import detect_peaks
    L = _hip.lib()
    for key in names(ref, "peaks"):
        for p in (1, 0):
            if key + "/img" not in ref:
                img = G.hashed((1080, 1920), int(ref[key + "/salt"])) // 16
                assert matches(ref, key, "peaks_%d" % p, detect_peaks(img, bool(p))), (key, p)
                continue
            img = ref[key + "/img"]
            if img.ndim == 2:
                assert matches(ref, key, "peaks_%d" % p, detect_peaks(img, bool(p))), (key, p)
                continue
            n, h, w = img.shape                     # a batch through the C ABI
            got = ops._pointwise_u8(L.va_detect_peaks_u8, np.ascontiguousarray(img), img.shape, n, h, w, p, None)
            assert matches(ref, key, "peaks_%d" % p, got.astype(bool)), (key, p)


def test_filter_normalize(ref):
    """normalize_u8_kernel and va_normalize: integer and one-ulp-below landings, learnt bounds applied to
    later frames outside them, float32 frames in float32; iteration and get_frame"""
    from video.filters import FilterNormalize
    from video.io.memory import VideoMemory
    for key in names(ref, "normalize"):
        frames = ref[key + "/frames"]
        vmin, vmax = float(ref[key + "/vmin"]), float(ref[key + "/vmax"])
        if frames.dtype == np.uint8:
            vmin, vmax = (None if np.isnan(v) else int(v) for v in (vmin, vmax))
        else:
            vmin, vmax = (None if np.isnan(v) else v for v in (vmin, vmax))
        dt = str(ref[key + "/dtype"]) or None
        filt = FilterNormalize(VideoMemory(frames), vmin, vmax, dt)
        assert matches(ref, key, "out", np.stack(list(filt))), key
        filt = FilterNormalize(VideoMemory(frames), vmin, vmax, dt)
        got = [filt.get_frame(0)] + [filt.get_frame(i) for i in range(len(frames) - 1, 0, -1)][::-1]
        assert matches(ref, key, "out", np.stack(got)), key


def test_filter_crop_and_monochrome(ref):
    """FilterCrop (nested, channels, alignment) per filter and contracted into the engine's prepare
    kernel; FilterMonochrome's mean on the GPU; both iteration and get_frame"""
    from video.filters import FilterMonochrome, FilterThreshold
    from video.io.memory import VideoMemory
    for key in names(ref, "crop"):
        src = str(ref[key + "/source"])
        frames = ref["crop_source/" + src]
        video = VideoMemory(frames) if src != "col4" else _video(frames)
        filt = build_crop(ref, key, video)
        assert filt.rect == tuple(int(v) for v in ref[key + "/rect"]), key
        assert matches(ref, key, "out", np.stack([np.array(f) for f in filt])), key
        assert matches(ref, key, "out", np.stack([filt.get_frame(i) for i in range(len(frames))])), key
        out = ref[key + "/out"]
        if out.ndim == 3 and src != "col4":         # a single-channel result: through the prepare kernel
            thr = FilterThreshold(build_crop(ref, key, VideoMemory(frames)), 127)
            assert thr._runner() is not None and thr._runner().engine.prepare is not None, key
            want = np.where(out > 127, 255, 0).astype(np.uint8)
            assert np.array_equal(np.stack([np.array(f) for f in thr]), want), key
            assert np.array_equal(thr.get_frame(1), want[1]), key
    for key in names(ref, "mono"):
        src, mode = str(ref[key + "/source"]), str(ref[key + "/mode"])
        frames = ref["crop_source/" + src]
        if src == "col4":
            if mode == "mean":                      # refused on the GPU path
                with pytest.raises(ValueError):
                    FilterMonochrome(_video(frames), mode).get_frame(0)
                continue
            filt = FilterMonochrome(_video(frames), mode)
        else:
            filt = FilterMonochrome(VideoMemory(frames), mode)
        assert matches(ref, key, "out", np.stack([np.array(f) for f in filt])), key
        assert matches(ref, key, "out", np.stack([filt.get_frame(i) for i in range(len(frames))])), key
        if mode == "mean":
            thr = FilterThreshold(FilterMonochrome(VideoMemory(frames), mode), 127)
            assert thr._runner() is not None and thr._runner().engine.prepare is not None
            want = np.where(ref[key + "/out"] > 127, 255, 0).astype(np.uint8)
            assert np.array_equal(np.stack([np.array(f) for f in thr]), want), key


def test_filter_time_difference(ref):
    from video.filters import FilterTimeDifference
    from video.io.memory import VideoMemory
    frames = ref["timediff/u8/frames"]
    td = FilterTimeDifference(VideoMemory(frames))
    assert matches(ref, "timediff/u8", "out", np.stack([np.array(f) for f in td]))
    td = FilterTimeDifference(VideoMemory(frames))
    assert matches(ref, "timediff/u8", "out", np.stack([td.get_frame(i) for i in range(len(frames) - 1)]))
    for dtype in (None, np.int32):                 # refused on the GPU path (int16 differences only)
        with pytest.raises(TypeError):
            FilterTimeDifference(VideoMemory(frames), dtype=dtype)
