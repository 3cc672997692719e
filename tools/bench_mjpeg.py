#!/usr/bin/env python3
"""Time of the Motion-JPEG encoder on the GPU (va_jpeg_encode_u8, va_jpeg.hip) and of the writer behind the composer:
  kernels   n x 1080p frames, monochrome and RGB, quality 90, resident on the device: the three launches by HIP
            events, next to a device-to-device copy of the same input bytes measured in the same run; the bytes out
            per frame.  Two contents: a smooth scene with mild noise (what a camera sees) and uniform noise (the
            worst case: the stream is about as large as the frames)
  encode    ops.jpeg_encode on a resident stack, wall clock with its downloads, next to the download of the raw
            frames that it replaces
  composer  VideoComposer end to end into an AVI file (a tracker's calls, as tools/bench_composer.py makes them),
            next to the same calls with sink=None, which downloads every frame uncompressed; same process, same clip
  pillow    Pillow's encoder (libjpeg) on one core, a few frames, where Pillow exists
  sampling  (--sampling: this leg alone) the RGB clips in 4:4:4, 4:2:2 and 4:2:0 (va_jpeg_encode_sampled_u8) in one
            run: the three launches by HIP events on resident data, the device copy, the bytes per frame, and
            ops.jpeg_encode with its download for each layout
  optimize  (--optimize: this leg alone) monochrome and the three colour layouts with the Annex K tables and with
            tables made for the call (va_jpeg_encode_optimized_u8; DESIGN.md §9, "Optimised Huffman tables") in one
            run: both calls by HIP events on resident data, the table kernel alone (va_jpeg_optimal_tables on the four
            tables of the fixture's largest file), the bytes per frame of both, Pillow's own optimised / plain ratio
            on frame 0 as tests/golden/mjpeg_optimized_v1.npz stores it, and ops.jpeg_encode with its download for
            both modes
Times are the median of the repetitions.  One JSON line per leg, appended to profiles/mjpeg_bench.jsonl (or --out);
a leg that did not run is written "not measured".
Run on an MI355X:
    python tools/bench_mjpeg.py [--reps 15] [--frames 256] [--sampling | --optimize]"""
import argparse
import io
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
ap.add_argument("--quality", type=int, default=90)
ap.add_argument("--cpu-frames", type=int, default=4, help="frames of the Pillow leg (0: not measured)")
ap.add_argument("--legs", default="kernels,encode,composer,pillow")
ap.add_argument("--sampling", action="store_true", help="run the sampling leg, and nothing else")
ap.add_argument("--optimize", action="store_true", help="run the optimize leg, and nothing else")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mjpeg_bench.jsonl"))
args = ap.parse_args()
LEGS = {"sampling"} if args.sampling else {"optimize"} if args.optimize else set(args.legs.split(","))
N, H, W, Q = args.frames, args.height, args.width, args.quality


def scene(n, h, w, c, rng, noise):
    """n frames: uniform noise, or a smooth moving pattern with discs and +-4 of noise"""
    shape = (n, h, w) + ((3,) if c == 3 else ())
    if noise:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    yy, xx = np.mgrid[:h, :w]
    base = 128 + 60 * np.sin(xx / 97.0) * np.cos(yy / 71.0)
    for _ in range(12):
        cx, cy, r = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(h / 40, h / 10)
        base[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] += rng.uniform(-60, 60)
    out = np.empty(shape, np.uint8)
    for t in range(n):
        plane = np.roll(base, 3 * t, axis=1) + rng.integers(-4, 5, (h, w))
        plane = np.clip(plane, 0, 255).astype(np.uint8)
        out[t] = plane if c == 1 else np.stack([plane, np.roll(plane, 5, axis=0), 255 - plane], axis=-1)
    return out


def main():
    import torch
    dev = torch.device("cuda", 0)
    S = torch.cuda.current_stream(dev).cuda_stream
    from video import _hip, ops
    from video.io.composer import VideoComposer
    L, check = _hip.lib(), _hip.check
    rng = np.random.default_rng(43)
    rows = []

    def emit(row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    def events(call):
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
        return float(np.median(ms))

    clips = {}
    for c in (1, 3):
        for noise in (False, True):
            if LEGS & {"kernels", "encode", "pillow"}:
                clips[(c, noise)] = scene(N, H, W, c, rng, noise)
    for (c, noise), clip in clips.items():
        name = "%s/%s" % ("rgb" if c == 3 else "mono", "noise" if noise else "smooth")
        raw = clip.nbytes
        if "kernels" in LEGS:
            frames = torch.from_numpy(clip).to(dev)
            head = np.frombuffer(ops.jpeg_header(H, W, c, Q), np.uint8)
            consts = torch.from_numpy(np.concatenate(ops.jpeg_tables(Q) + (head,))).to(dev)
            info = torch.zeros(2 * N + 2, dtype=torch.int64, device=dev)
            cap = raw + N * 4096
            out = torch.empty(cap, dtype=torch.uint8, device=dev)
            run = lambda: check(L.va_jpeg_encode_u8(frames.data_ptr(), N, H, W, c, consts.data_ptr(),
                                                    consts.data_ptr() + 128, len(head), info.data_ptr() + 16 + 8 * N,
                                                    info.data_ptr() + 8, info.data_ptr(), out.data_ptr(), cap, S))
            best, med = events(run)
            total = int(info[0])
            assert total <= cap
            twin = torch.empty_like(frames)
            _, copy_med = events(lambda: twin.copy_(frames))
            del twin, out
            emit({"leg": "kernels/" + name, "frames": N, "h": H, "w": W, "quality": Q, "ms_per_call_min": round(best, 4),
                  "ms_per_call_median": round(med, 4), "frames_per_s": round(N / med * 1e3, 1),
                  "input_gb_per_s": round(raw / med / 1e6, 1), "bytes_out_per_frame": total // N,
                  "raw_bytes_per_frame": raw // N, "compression": round(raw / total, 2),
                  "memcpy_same_input_ms_median": round(copy_med, 4), "times_the_memcpy": round(med / copy_med, 2),
                  "note": "count + scan + write launches; every segment is encoded twice"})
            del frames
        if "encode" in LEGS:
            stack = ops.DeviceFrames.upload(clip)
            enc = wall(lambda: ops.jpeg_encode(stack, Q, ret_packed=True), args.reps)
            down = wall(lambda: stack.download(), args.reps)
            blob, _ = ops.jpeg_encode(stack, Q, ret_packed=True)
            stack.release()
            emit({"leg": "encode/" + name, "frames": N, "h": H, "w": W, "quality": Q,
                  "jpeg_encode_with_downloads_ms_median": round(enc, 2), "raw_download_ms_median": round(down, 2),
                  "bytes_downloaded": int(len(blob)), "raw_bytes": raw, "frames_per_s": round(N / enc * 1e3, 1),
                  "note": "wall clock on a resident stack; the raw download is into a fresh pageable array"})
        if "pillow" in LEGS:
            row = {"leg": "pillow/" + name, "frames": args.cpu_frames, "quality": Q}
            try:
                from PIL import Image
            except ImportError:
                Image = None
            if Image is None or not args.cpu_frames:
                row["ms_per_frame"] = "not measured"
            else:
                t0, size = time.perf_counter(), 0
                for f in clip[:args.cpu_frames]:
                    buf = io.BytesIO()
                    Image.fromarray(f).save(buf, "JPEG", quality=Q, subsampling=0, optimize=False)
                    size += buf.tell()
                row.update({"ms_per_frame": round((time.perf_counter() - t0) * 1e3 / args.cpu_frames, 2),
                            "bytes_out_per_frame": size // args.cpu_frames, "note": "libjpeg through Pillow, one core, 4:4:4"})
            emit(row)
    clips.clear()
    if "sampling" in LEGS:
        for noise in (False, True):
            clip = scene(N, H, W, 3, rng, noise)
            raw = clip.nbytes
            frames = torch.from_numpy(clip).to(dev)
            twin = torch.empty_like(frames)
            _, copy_med = events(lambda: twin.copy_(frames))
            del twin
            info = torch.zeros(2 * N + 2, dtype=torch.int64, device=dev)
            cap = raw + N * 4096
            out = torch.empty(cap, dtype=torch.uint8, device=dev)
            stack = ops.DeviceFrames.upload(clip)
            base = None
            for layout, (hh, vv) in ops.JPEG_SAMPLINGS.items():
                head = np.frombuffer(ops.jpeg_header(H, W, 3, Q, (hh, vv)), np.uint8)
                consts = torch.from_numpy(np.concatenate(ops.jpeg_tables(Q) + (head,))).to(dev)
                tail = (consts.data_ptr(), consts.data_ptr() + 128, len(head), info.data_ptr() + 16 + 8 * N,
                        info.data_ptr() + 8, info.data_ptr(), out.data_ptr(), cap, S)
                if (hh, vv) == (1, 1):
                    run = lambda: check(L.va_jpeg_encode_u8(frames.data_ptr(), N, H, W, 3, *tail))
                else:
                    run = lambda: check(L.va_jpeg_encode_sampled_u8(frames.data_ptr(), N, H, W, 3, hh, vv, *tail))
                best, med = events(run)
                total = int(info[0])
                assert total <= cap
                base = med if base is None else base
                enc = wall(lambda: ops.jpeg_encode(stack, Q, ret_packed=True, sampling=(hh, vv)), args.reps)
                emit({"leg": "sampling/rgb/%s/%s" % ("noise" if noise else "smooth", layout), "frames": N, "h": H, "w": W,
                      "quality": Q, "ms_per_call_min": round(best, 4), "ms_per_call_median": round(med, 4),
                      "of_the_444_time": round(med / base, 3), "frames_per_s": round(N / med * 1e3, 1),
                      "bytes_out_per_frame": total // N, "raw_bytes_per_frame": raw // N,
                      "memcpy_same_input_ms_median": round(copy_med, 4), "times_the_memcpy": round(med / copy_med, 2),
                      "jpeg_encode_with_downloads_ms_median": round(enc, 2),
                      "note": "count + scan + write launches by HIP events on resident frames; 4:4:4, the copy and the "
                              "other layouts in one run; jpeg_encode: wall clock on a resident stack"})
            stack.release()
            del frames, out
    if "optimize" in LEGS:
        z = np.load(os.path.join(ROOT, "tests", "golden", "mjpeg_optimized_v1.npz"))
        pillow = {str(k): [int(x) for x in v] for k, v in zip(z["ratio_names"], z["ratio_bytes"])}
        at = int(np.argmax(z["pin_counts"].reshape(-1, 256).sum(axis=1))) // 4 * 4    # (colour files come first, 4 tables each)
        counts = torch.from_numpy(z["pin_counts"][at:at + 4].astype(np.int64)).to(dev)
        tables = torch.zeros(4 * ops.JPEG_TABLE_BYTES, dtype=torch.uint8, device=dev)
        _, table_med = events(lambda: check(L.va_jpeg_optimal_tables(counts.data_ptr(), 4, tables.data_ptr(), S)))
        for noise in (False, True):
            for c in (1, 3):
                clip = scene(N, H, W, c, np.random.default_rng(47 + noise), noise)   # (frame 0: the fixture generator's)
                raw = clip.nbytes
                frames = torch.from_numpy(clip).to(dev)
                info = torch.zeros(2 * N + 2, dtype=torch.int64, device=dev)
                cap = raw + N * 4096
                out = torch.empty(cap, dtype=torch.uint8, device=dev)
                stack = ops.DeviceFrames.upload(clip)
                for layout, (hh, vv) in ([("mono", (1, 1))] if c == 1 else
                                         [(k.replace(":", ""), v) for k, v in ops.JPEG_SAMPLINGS.items()]):
                    head = ops.jpeg_header(H, W, c, Q, (hh, vv))
                    pre, post = ops.jpeg_header_pieces(head)
                    consts = torch.from_numpy(np.concatenate(ops.jpeg_tables(Q) + tuple(
                        np.frombuffer(b, np.uint8) for b in (head, pre, post)))).to(dev)
                    qt, at_pre = consts.data_ptr(), consts.data_ptr() + 128 + len(head)
                    tail = (info.data_ptr() + 16 + 8 * N, info.data_ptr() + 8, info.data_ptr(), out.data_ptr(), cap, S)
                    plain = lambda: check(L.va_jpeg_encode_sampled_u8(frames.data_ptr(), N, H, W, c, hh, vv, qt, qt + 128,
                                                                      len(head), *tail))
                    optimised = lambda: check(L.va_jpeg_encode_optimized_u8(
                        frames.data_ptr(), N, H, W, c, hh, vv, qt, at_pre, len(pre), at_pre + len(pre), len(post),
                        tables.data_ptr(), *tail))
                    _, plain_med = events(plain)
                    plain_total = int(info[0])
                    _, opt_med = events(optimised)
                    opt_total = int(info[0])
                    assert plain_total <= cap and opt_total <= plain_total
                    enc = {flag: wall(lambda: ops.jpeg_encode(stack, Q, ret_packed=True, sampling=(hh, vv), optimize=flag),
                                      args.reps) for flag in (False, True)}
                    name = "%s/%s" % ("noise" if noise else "smooth", layout)
                    emit({"leg": "optimize/" + name, "frames": N, "h": H, "w": W, "quality": Q,
                          "plain_ms_per_call_median": round(plain_med, 4), "optimized_ms_per_call_median": round(opt_med, 4),
                          "of_the_plain_time": round(opt_med / plain_med, 3), "table_kernel_ms_median": round(table_med, 4),
                          "plain_bytes_per_frame": plain_total // N, "optimized_bytes_per_frame": opt_total // N,
                          "of_the_plain_bytes": round(opt_total / plain_total, 4),
                          "pillow_frame0_plain_optimized_bytes": pillow[name],
                          "pillow_of_the_plain_bytes": round(pillow[name][1] / pillow[name][0], 4),
                          "jpeg_encode_with_downloads_ms_median": round(enc[False], 2),
                          "jpeg_encode_optimized_with_downloads_ms_median": round(enc[True], 2),
                          "note": "both calls by HIP events on resident frames in one run; the optimised call: zero, "
                                  "histogram, tables, count, scan, write; the table kernel alone on 4 tables; jpeg_encode: "
                                  "wall clock on a resident stack"})
                stack.release()
                del frames, out
    if "composer" in LEGS:
        rng = np.random.default_rng(41)
        for noise in (False, True):
            clip = scene(N, H, W, 1, rng, noise)
            background = scene(1, H, W, 3, rng, noise)[0]
            yy, xx = np.mgrid[:H, :W]
            masks = [((xx - (200 + 5 * t)) ** 2 + (yy - 500) ** 2 <= 150 ** 2).astype(np.uint8) for t in range(8)]

            def calls(target, t):
                r = np.random.default_rng(t)
                target.set_frame(clip[t])
                target.highlight_mask(masks[t % 8], "g", 128)
                target.blend_image(background, 0.3)
                target.add_line(np.cumsum(r.integers(-40, 41, (20, 2)), axis=0) + (W // 2, H // 2), "b", is_closed=False)
                target.add_rectangle((100 + t, 80, 300, 200), "y")
                target.add_points(r.integers(1, min(H, W), (200, 2)), 1, "w")

            def run(sink):
                vc = VideoComposer(sink, (W, H), 25, True, batch=32)
                for t in range(N):
                    calls(vc, t)
                vc.close()
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, "bench.avi")
                to_file = wall(lambda: run(path), 3)
                size = os.path.getsize(path)
            to_none = wall(lambda: run(None), 3)
            emit({"leg": "composer/%s" % ("noise" if noise else "smooth"), "frames": N, "h": H, "w": W, "quality": Q,
                  "into_avi_file_ms_median": round(to_file, 1), "into_avi_file_frames_per_s": round(N / to_file * 1e3, 1),
                  "sink_none_ms_median": round(to_none, 1), "sink_none_frames_per_s": round(N / to_none * 1e3, 1),
                  "file_bytes": size, "raw_bytes": N * H * W * 3,
                  "note": "wall clock, RGB output: recording, capture copies, uploads, both passes, then either the "
                          "encoder, the download of the stream and the file writes, or the download of the raw frames"})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


main()
