#!/usr/bin/env python3
"""Time of the composer passes on the GPU (va_compose_layers_u8, va_draw_u8, va_compose.hip) and of VideoComposer:
  layers    n x 1080p frames, monochrome and RGB, in place: one highlight per frame (its own mask), and highlight +
            blend with one background image; HIP events on resident data, reported as bytes moved per second next to
            a device-to-device copy of the same number of bytes measured in the same run
  draw      n x 1080p frames with the contours of a blob clip, 200 points and 10 polylines per frame, next to
            va_find_contours on the same stack (drawing the contours back should not cost more than finding them)
  composer  VideoComposer end to end (wall clock, uploads and downloads included) on n frames with a tracker's calls,
            next to the NumPy restatement tests/composer_checks.py on one core (a few frames, extrapolated)
Times are the median of the repetitions.  One JSON line per leg, appended to profiles/composer_bench.jsonl (or
--out); a leg that did not run is written "not measured".
Run on an MI355X:
    python tools/bench_composer.py [--reps 15] [--frames 256]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "video-analysis_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--cpu-frames", type=int, default=2, help="frames of the restatement leg (0: not measured)")
ap.add_argument("--legs", default="layers,draw,composer", help="which of layers, draw and composer run")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "composer_bench.jsonl"))
args = ap.parse_args()
LEGS = set(args.legs.split(","))
N, H, W = args.frames, args.height, args.width


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


def blob_masks(n, h, w, rng):
    """n masks of moving discs: 8 base masks, shifted"""
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


def frame_commands(contours, rng, h, w, c):
    white, red = (255 if c == 1 else (255, 255, 255)), (200 if c == 1 else (255, 0, 0))
    cmds = [("polyline", k, True, red) for k in contours]
    cmds += [("circle", (int(rng.integers(0, w)), int(rng.integers(0, h))), 1, True, white) for _ in range(200)]
    for _ in range(10):
        pts = np.cumsum(rng.integers(-40, 41, (20, 2)), axis=0) + (rng.integers(0, w), rng.integers(0, h))
        cmds.append(("polyline", pts, False, white))
    return cmds


def main():
    import torch
    dev = torch.device("cuda", 0)
    S = torch.cuda.current_stream(dev).cuda_stream
    from video import _hip, ops
    from video.io.composer import VideoComposer, get_color
    import composer_checks as K
    L, check = _hip.lib(), _hip.check
    rng = np.random.default_rng(41)
    rows = []
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def emit(row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    masks = blob_masks(N, H, W, rng)
    if "layers" in LEGS:
        dmasks = up(masks)
        for c in (1, 3):
            shape = (N, H, W) + ((3,) if c == 3 else ())
            frames = torch.randint(0, 256, shape, dtype=torch.uint8, device=dev)
            image = rng.integers(0, 256, shape[1:], dtype=np.uint8)
            for name, with_blend in (("highlight", False), ("highlight+blend", True)):
                # (the tables are built with one mask and then pointed at the resident per-frame masks)
                layers = [[("highlight", masks[0], "g" if c == 3 else "all", 128)] +
                          ([("blend", image, 0.3, None)] if with_blend else []) for f in range(N)]
                table, off, images, _ = ops._compose_tables(layers, N, H, W, c, "bench")
                table["mask_off"] = [f * H * W for f in range(N) for _ in range(1 + with_blend)]
                if with_blend:
                    table["mask_off"][1::2] = -1
                dt, do = up(table.view(np.uint8)), up(off)
                di = up(images) if images is not None else None
                best, med = timed(lambda: check(L.va_compose_layers_u8(
                    frames.data_ptr(), c, frames.data_ptr(), N, H, W, c, dt.data_ptr(), do.data_ptr(), len(table),
                    di.data_ptr() if di is not None else None, 0 if images is None else len(images), dmasks.data_ptr(),
                    dmasks.numel(), S)), torch)
                moved = N * H * W * (2 * c + 1 + (c if with_blend else 0))
                a, b = (torch.empty(moved // 2, dtype=torch.uint8, device=dev) for _ in range(2))
                _, copy_med = timed(lambda: b.copy_(a), torch)
                del a, b
                emit({"leg": "layers/%s/%s" % ("rgb" if c == 3 else "mono", name), "frames": N, "h": H, "w": W,
                      "ms_per_call_min": round(best, 4), "ms_per_call_median": round(med, 4), "bytes_moved": moved,
                      "gb_per_s": round(moved / med / 1e6, 1), "memcpy_same_bytes_ms_median": round(copy_med, 4),
                      "memcpy_gb_per_s": round(moved / copy_med / 1e6, 1), "fraction_of_memcpy": round(copy_med / med, 3),
                      "frames_per_s": round(N / med * 1e3, 1),
                      "note": "bytes moved: the frame read and written, its mask, and the image once per frame"})
            del frames
    contours = None
    if "draw" in LEGS or "composer" in LEGS:
        contours = []
        for lo in range(0, N, 32):
            contours += ops.find_contours(masks[lo:lo + 32])
    if "draw" in LEGS:
        dmasks = up(masks)
        ws_bytes = L.va_find_contours_workspace_bytes(N, H, W)
        k, npts = sum(len(cs) for cs in contours), sum(len(c) for cs in contours for c in cs)
        ws, ncb, tot = (torch.empty(max(b, 16), dtype=torch.uint8, device=dev) for b in (ws_bytes, N * 4, 16))
        info, offb, pts = (torch.empty(max(b, 16), dtype=torch.uint8, device=dev)
                           for b in (k * ops.CONTOUR_INFO_DTYPE.itemsize, (k + 1) * 8, npts * 8))
        fbest, fmed = timed(lambda: check(L.va_find_contours(dmasks.data_ptr(), N, H, W, ncb.data_ptr(), tot.data_ptr(),
                                                             info.data_ptr(), offb.data_ptr(), k, pts.data_ptr(), npts,
                                                             ws.data_ptr(), ws_bytes, S)), torch)
        for c in (1, 3):
            shape = (N, H, W) + ((3,) if c == 3 else ())
            frames = torch.randint(0, 256, shape, dtype=torch.uint8, device=dev)
            for name, only_contours in (("contours", True), ("contours+200points+10polylines", False)):
                r = np.random.default_rng(7)
                commands = [[x for x in frame_commands(cs, r, H, W, c) if only_contours <= (x[0] == "polyline" and x[2])]
                            for cs in contours]
                table, off, points = ops._draw_tables(commands, N, c, "bench")
                dt, do, dp = up(table.view(np.uint8)), up(off), up(points)
                st = torch.empty(N, dtype=torch.int32, device=dev)
                best, med = timed(lambda: check(L.va_draw_u8(frames.data_ptr(), N, H, W, c, dt.data_ptr(), do.data_ptr(),
                                                             len(table), dp.data_ptr(), len(points), st.data_ptr(), S)),
                                  torch)
                assert int(st.abs().sum()) == 0
                emit({"leg": "draw/%s/%s" % ("rgb" if c == 3 else "mono", name), "frames": N, "h": H, "w": W,
                      "commands": len(table), "points": len(points), "ms_per_call_min": round(best, 4),
                      "ms_per_call_median": round(med, 4), "frames_per_s": round(N / med * 1e3, 1),
                      "find_contours_same_stack_ms_median": round(fmed, 4), "find_contours_ms_min": round(fbest, 4)})
            del frames
    if "composer" in LEGS:
        clip = rng.integers(0, 256, (N, H, W), dtype=np.uint8)
        background = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)

        def calls(target, t):
            r = np.random.default_rng(t)
            target.set_frame(clip[t])
            target.highlight_mask(masks[t], "g", 128)
            target.blend_image(background, 0.3)
            target.add_contour(contours[t], "r")
            target.add_line(np.cumsum(r.integers(-40, 41, (20, 2)), axis=0) + (W // 2, H // 2), "b", is_closed=False)
            target.add_rectangle((100 + t, 80, 300, 200), "y")
            target.add_points(r.integers(1, min(H, W), (200, 2)), 1, "w")

        def run():
            vc = VideoComposer(lambda frame: None, (W, H), 25, True, batch=32)
            for t in range(N):
                calls(vc, t)
            vc.close()
        run()
        ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            run()
            ms.append((time.perf_counter() - t0) * 1e3)
        row = {"leg": "composer/end_to_end", "frames": N, "h": H, "w": W, "ms_median": round(float(np.median(ms)), 1),
               "frames_per_s": round(N / np.median(ms) * 1e3, 1),
               "note": "wall clock: recording, capture copies, uploads, both passes, the download"}
        if args.cpu_frames:
            rp = K.Replay((W, H), True, get_color=get_color)
            t0 = time.perf_counter()
            for t in range(args.cpu_frames):
                calls(rp, t)
            rp.close()
            per = (time.perf_counter() - t0) * 1e3 / args.cpu_frames
            row.update({"numpy_restatement_one_core_ms_per_frame": round(per, 1), "restatement_frames": args.cpu_frames,
                        "restatement_ms_extrapolated": round(per * N, 1)})
        else:
            row["numpy_restatement_one_core_ms_per_frame"] = "not measured"
        emit(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


main()
