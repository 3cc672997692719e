#!/usr/bin/env python3
"""Time of annotating on the device (va_draw_contours_u8, va_compose.hip; VideoComposer.annotate_frames):
  kernel    the contours of a blob clip drawn into n x 1080p frames by va_draw_contours_u8 (chip-wide, a lane per
            point) and by va_draw_u8 (a workgroup per frame) from the same va_find_contours result, in one run:
            n = --frames and n = 32 (one flush of the composer), monochrome and RGB; HIP events on resident data
  e2e       frames resident on the device, in stacks of 32: FrameEngine.run_frames(keep=("mask",)) ->
            ops.find_contours(keep=True) -> VideoComposer.annotate_frames into a sink that discards the stacks and
            into a Motion-JPEG file, next to the per-frame composer loop over the same clip in the same process
            (masks downloaded, host contour lists, set_frame / highlight_mask / add_contour), and one pass of the
            device path with the wall clock of each stage
Times are the median of the repetitions.  One JSON line per leg, appended to profiles/annotate_bench.jsonl (or
--out).  The tool asserts nothing about speed.
Run on an MI355X:
    python tools/bench_annotate.py [--reps 15] [--frames 256]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "video-analysis_amd"))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--legs", default="kernel,e2e", help="which of kernel and e2e run")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "annotate_bench.jsonl"))
args = ap.parse_args()
LEGS = set(args.legs.split(","))
N, H, W = args.frames, args.height, args.width
FLUSH = 32


def timed(call, torch):
    call()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(args.reps):
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return min(ms), float(np.median(ms))


def wall(call, reps):
    call()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return min(ms), float(np.median(ms))


def blob_masks(n, h, w, rng):
    """n masks of moving discs: 8 base masks, shifted (the clip of tools/bench_composer.py)"""
    yy, xx = np.mgrid[:h, :w]
    base = []
    for _ in range(8):
        m = np.zeros((h, w), bool)
        for _ in range(6):
            cx, cy, r = rng.uniform(0.1, 0.9) * w, rng.uniform(0.1, 0.9) * h, rng.uniform(h / 30 + 2, h / 8 + 3)
            m |= (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r
        m[[0, -1]] = m[:, [0, -1]] = False
        base.append(m.astype(np.uint8))
    return np.stack([np.roll(base[t % 8], (3 * t) % (w // 4), axis=1) for t in range(n)])


class Discard(object):
    """a sink that takes the finished stacks and drops them"""
    stacks = 0

    def write_frames(self, stack):
        self.stacks += 1


def main():
    import torch
    dev = torch.device("cuda", 0)
    S = torch.cuda.current_stream(dev).cuda_stream
    from video import _hip, ops
    from video.engine import FrameEngine
    from video.io.composer import VideoComposer
    L, check = _hip.lib(), _hip.check
    rng = np.random.default_rng(41)
    rows = []

    def emit(row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    masks = blob_masks(N, H, W, rng)
    if "kernel" in LEGS:
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        for n in sorted({N, min(N, FLUSH)}, reverse=True):
            held = ops.DeviceFrames.upload(masks[:n])
            found = ops.find_contours(held, keep=True)
            lists = found.download()
            seg = np.concatenate([np.abs(np.roll(c, -1, axis=0) - c).reshape(-1, 2).max(axis=1)
                                  for cs in lists for c in cs])
            for c in (1, 3):
                shape = (n, H, W) + ((3,) if c == 3 else ())
                frames = torch.randint(0, 256, shape, dtype=torch.uint8, device=dev)
                color = 200 if c == 1 else (255, 0, 0)
                packed = ops._draw_color(color, c, "bench")
                st = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
                best, med = timed(lambda: check(L.va_draw_contours_u8(
                    frames.data_ptr(), n, H, W, c, found.info.ptr, found.point_off.ptr, found.ncontours, found.points.ptr,
                    found.npoints, None, n, packed, st.data_ptr(), S)), torch)
                assert int(st[0]) == 0
                after_new = frames.clone()
                table, off, points = ops._draw_tables([[("polyline", k, True, color) for k in cs] for cs in lists], n, c,
                                                      "bench")
                dt, do, dp = up(table.view(np.uint8)), up(off), up(points)
                obest, omed = timed(lambda: check(L.va_draw_u8(frames.data_ptr(), n, H, W, c, dt.data_ptr(), do.data_ptr(),
                                                               len(table), dp.data_ptr(), len(points), st.data_ptr(), S)),
                                    torch)
                assert int(st.abs().sum()) == 0 and bool((frames == after_new).all())     # the two draw the same bytes
                emit({"leg": "kernel/%s/%d_frames" % ("rgb" if c == 3 else "mono", n), "frames": n, "h": H, "w": W,
                      "contours": found.ncontours, "points": found.npoints,
                      "segment_pixels_mean": round(float(seg.mean()) + 1, 2), "segment_pixels_max": int(seg.max()) + 1,
                      "draw_contours_ms_min": round(best, 4), "draw_contours_ms_median": round(med, 4),
                      "draw_u8_same_contours_ms_min": round(obest, 4), "draw_u8_same_contours_ms_median": round(omed, 4),
                      "draw_u8_over_draw_contours": round(omed / med, 2),
                      "note": "same run, same contours, in place on resident frames; HIP events"})
                del frames, after_new
            found.release()
            held.release()
    if "e2e" in LEGS:
        clip = np.where(masks != 0, 190, 60).astype(np.uint8) + rng.integers(0, 20, (N, H, W), dtype=np.uint8)
        stacks = [ops.DeviceFrames.upload(clip[lo:lo + FLUSH]) for lo in range(0, N, FLUSH)]
        eng = FrameEngine(size=(W, H), max_batch=FLUSH, sigma=2.0, thresh=125)
        tmp = tempfile.mkdtemp(prefix="annotate_bench_")
        stages = {}

        def device_path(sink, clock=None):
            vc = VideoComposer(sink, (W, H), 25, True, batch=FLUSH)
            for stack in stacks:
                t0 = time.perf_counter()
                mask = eng.run_frames(stack, want=(), keep=("mask",))["mask"]
                t1 = time.perf_counter()
                found = ops.find_contours(mask, keep=True)
                t2 = time.perf_counter()
                if clock is not None:
                    clock["contours"] = clock.get("contours", 0) + found.ncontours
                    clock["points"] = clock.get("points", 0) + found.npoints
                vc.annotate_frames(stack, mask, "g", 128, contours=found, color="r")
                t3 = time.perf_counter()
                found.release()
                mask.release()
                if clock is not None:
                    for name, ms in (("engine_keep_mask", t1 - t0), ("find_contours_keep", t2 - t1),
                                     ("annotate_frames", t3 - t2)):
                        clock[name] = clock.get(name, 0.0) + ms * 1e3
            vc.close()
            return vc.frames_written

        def per_frame_path(sink):
            vc = VideoComposer(sink, (W, H), 25, True, batch=FLUSH)
            for stack in stacks:
                mask = eng.run_frames(stack, want=("mask",))["mask"]
                lists = ops.find_contours(mask)
                frames = stack.download()
                for i in range(len(frames)):
                    vc.set_frame(frames[i])
                    vc.highlight_mask(mask[i], "g", 128)
                    vc.add_contour(lists[i], "r")
            vc.close()
            return vc.frames_written

        assert device_path(Discard()) == N and per_frame_path(Discard()) == N
        for name, sink in (("discard", Discard), ("mjpeg_file", lambda: os.path.join(tmp, "out.avi"))):
            dbest, dmed = wall(lambda: device_path(sink()), args.reps)
            pbest, pmed = wall(lambda: per_frame_path(sink()), args.reps)
            emit({"leg": "e2e/%s" % name, "frames": N, "h": H, "w": W, "flush": FLUSH, "video": "rgb",
                  "device_path_ms_min": round(dbest, 1), "device_path_ms_median": round(dmed, 1),
                  "device_path_frames_per_s": round(N / dmed * 1e3, 1),
                  "per_frame_loop_ms_min": round(pbest, 1), "per_frame_loop_ms_median": round(pmed, 1),
                  "per_frame_loop_frames_per_s": round(N / pmed * 1e3, 1),
                  "per_frame_over_device": round(pmed / dmed, 2),
                  "note": "wall clock, same process; frames resident in stacks of 32; the per-frame loop downloads the "
                          "frames and the masks and finds host contour lists"})
        device_path(Discard(), stages)
        emit({"leg": "e2e/discard/stages", "frames": N, "h": H, "w": W, "contours": stages.pop("contours"),
              "points": stages.pop("points"), "ms": {k: round(v, 1) for k, v in stages.items()},
              "note": "one pass of the device path, wall clock per stage, summed over the stacks"})
        eng.close()
        for s in stacks:
            s.release()
        for f in os.listdir(tmp):
            os.remove(os.path.join(tmp, f))
        os.rmdir(tmp)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


main()
