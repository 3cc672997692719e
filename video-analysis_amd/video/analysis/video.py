"""Temporal statistics of a video (reference: video/analysis/video.py:14-55).

measure_mean / measure_mean_std keep their float64 state on the GPU and fold frames in with
exactly the reference's arithmetic (`mean*n/(n+1) + frame/(n+1)`; Welford for the variance).
measure_median / measure_percentiles have no counterpart there: they sample up to 255 frames and take the exact
per-pixel ranks on the GPU ("Temporal median")."""
import numpy as np


def reduce_video(video, function, initial_value=None):
    """folds `function(frame, result)` over the frames (host callable)"""
    result = initial_value
    for frame in video:
        result = frame if result is None else function(frame, result)
    return result


_FRAME_DTYPES = (np.uint8, np.int16, np.float32, np.float64)


def _batches(video, batch):
    """stacks of `batch` frames; uint8, int16 (FilterTimeDifference), float32 and float64
    (FilterNormalize(dtype=np.float64)) videos"""
    buf = []
    for frame in video:
        frame = np.asarray(frame)
        if frame.dtype not in _FRAME_DTYPES:
            raise TypeError("the GPU path takes uint8, int16, float32 or float64 frames, got %s" % frame.dtype)
        buf.append(np.array(frame))
        if len(buf) == batch:
            yield np.stack(buf)
            buf = []
    if buf:
        yield np.stack(buf)


def measure_mean(video, batch=32):
    """mean of every pixel over time, float64 (reference :26-35)"""
    from .. import ops
    mean, n = None, 0
    model = None
    for frames in _batches(video, batch):
        if frames.dtype == np.uint8:            # device-resident state, division-free kernel
            if model is None:
                model = ops.BackgroundModel(video.shape[1:], "mean", dtype=np.uint8)
            model.process(frames, want_diff=False)
        else:                                   # int16 / float32 / float64 frames: NumPy's promotions restated
            mean = ops.running_mean(frames, mean, n)
        n += len(frames)
    if model is not None:
        return model.state
    return np.zeros(video.shape[1:]) if mean is None else mean


def measure_mean_std(video, batch=32):
    """mean and standard deviation of every pixel over time (reference :39-55)"""
    from .. import ops
    mean = m2 = None
    n = 0
    last = None
    for frames in _batches(video, batch):
        mean, m2 = ops.welford(frames, mean, m2, n)
        n += len(frames)
        last = frames[-1]
    if n == 0:
        raise ValueError("video is empty")
    if n - 1 < 2:                       # reference: `if n < 2` with n = last frame index
        return last, 0
    return mean, np.sqrt(m2 / (n - 1))


def sample_indices(frame_count, max_frames):
    """the frames measure_median and measure_percentiles use: all of them up to max_frames, otherwise max_frames of
    them spread evenly, (j * frame_count) // max_frames for j = 0 .. max_frames - 1"""
    if frame_count <= max_frames:
        return list(range(frame_count))
    return [(j * frame_count) // max_frames for j in range(max_frames)]


def _sampled_stack(video, max_frames, what):
    """the uint8 stack of the sampled frames; every argument check comes before the first frame is read"""
    from .. import ops
    if isinstance(max_frames, bool) or not isinstance(max_frames, (int, np.integer)) or \
            not 1 <= max_frames <= ops.TEMPORAL_MAX_PLANES:
        raise ValueError("%s: max_frames is an integer 1 .. %d, got %r" % (what, ops.TEMPORAL_MAX_PLANES, max_frames))
    if video.frame_count < 1:
        raise ValueError("%s: video is empty" % what)
    wanted = sample_indices(video.frame_count, int(max_frames))
    frames = []
    if video.seekable:
        pos = video.get_frame_pos()
        try:
            for k in wanted:
                frames.append(np.array(video.get_frame(k)))
        finally:
            video.set_frame_pos(pos)
    else:
        pending = iter(wanted)
        nxt = next(pending)
        for k, frame in enumerate(video):
            if k == nxt:
                frames.append(np.array(frame))
                nxt = next(pending, None)
                if nxt is None:
                    break
    if len(frames) != len(wanted):
        raise ValueError("%s: the video ended after %d of the %d sampled frames" % (what, len(frames), len(wanted)))
    for frame in frames:
        if frame.dtype != np.uint8:
            raise TypeError("%s takes uint8 frames, got %s" % (what, frame.dtype))
    return np.stack(frames)


def measure_median(video, max_frames=101):
    """np.median over time of every pixel of up to max_frames (<= 255) frames of a uint8 video spread evenly over it
    (sample_indices), float64: a background image without the ghost of what moved through the clip"""
    from .. import ops
    return ops.temporal_median(_sampled_stack(video, max_frames, "measure_median"))


def measure_percentiles(video, q, method="lower", max_frames=101):
    """np.percentile(..., q, axis=0, method=method) over the same sample, method 'lower', 'higher' or 'nearest':
    uint8 planes, one per q (q = 0 and 100: the minimum and maximum projections)"""
    from .. import ops
    if method not in ops.PERCENTILE_METHODS:
        raise ValueError("measure_percentiles: method is one of %r, got %r" % (ops.PERCENTILE_METHODS, method))
    return ops.temporal_percentiles(_sampled_stack(video, max_frames, "measure_percentiles"), q, method)
