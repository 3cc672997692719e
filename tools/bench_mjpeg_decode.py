#!/usr/bin/env python3
"""Time of the Motion-JPEG decoder on the GPU (va_jpeg_decode_u8, va_jpeg_decode.hip) and of the reader in front of it:
  kernels   n x 1080p frames, monochrome and RGB, quality 90, the encoder's own streams resident on the device: the
            call (locate + entropy + reconstruct per chunk) by HIP events, next to a device-to-device copy of its
            output and to va_jpeg_encode_u8 on the same frames, all in the same run.  The ABI enqueues its three
            launches together, so this leg cannot time them one by one; a run of this leg under
            `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/bench_mjpeg_decode.py --legs kernels`
            lists them per kernel.
            Two contents: a smooth scene with mild noise and uniform noise
  batch32   the same call on the first 32 frames: one lane per segment leaves most of the machine idle there
  ops       ops.jpeg_decode from host bytes, wall clock with its upload and the download of the frames, and with
            keep=True (no download), next to the upload of the raw pixels that it replaces
  pillow    Pillow's decoder (libjpeg) on one core, a few frames, where Pillow exists
  video     VideoMJPEG iteration end to end over an AVI file with the device decoder and, where Pillow exists, with
            the default one
  subsampled  n x 1080p RGB frames as Pillow (libjpeg) writes them at quality 90: 4:2:0 and 4:2:2 through
            va_jpeg_decode_sampled_u8 (locate + entropy + chroma planes + pixels) and 4:4:4 of the same pictures
            through va_jpeg_decode_u8, each with one restart interval per MCU row and with none (a frame is then one
            segment, one lane), by HIP events in the same run; the launches one by one come from the same
            rocprofv3 run as above with --legs subsampled.  Skipped with a message where Pillow is missing
  split     the Pillow-written pictures of the subsampled leg without restart markers (what cameras write), 4:4:4,
            4:2:2 and 4:2:0, at batches of 32 and --frames: the one-lane entries (ops.jpeg_decode(split=False), the
            only path before the split decoder existed) against va_jpeg_decode_split_u8 with ops' defaults, with the
            rounds its frames took; at --frames a sweep of sub_bytes over 128, 256, 512, 1024 and of max_rounds; the
            same pictures with a restart interval per MCU row next to them; and the routing crossover: both paths on
            batches of 32 square frames of 64 .. 512 pixels (entropy bytes per frame against time).  --split-brief
            runs only the default call (for a rocprofv3 --kernel-trace --stats run that lists its launches)
Times are the median of the repetitions.  One JSON line per leg, appended to profiles/mjpeg_decode_bench.jsonl (or
--out); a leg that did not run is written "not measured".
Run on an MI355X:
    python tools/bench_mjpeg_decode.py [--reps 15] [--frames 256]"""
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
ap.add_argument("--video-frames", type=int, default=64, help="frames of the VideoMJPEG leg")
ap.add_argument("--distinct", type=int, default=16, help="pictures of the subsampled leg, repeated to --frames")
ap.add_argument("--legs", default="kernels,batch32,ops,pillow,video,subsampled,split")
ap.add_argument("--split-brief", action="store_true", help="the split leg: only the default call at --frames")
ap.add_argument("--modes", default="mono,rgb")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mjpeg_decode_bench.jsonl"))
args = ap.parse_args()
LEGS = set(args.legs.split(","))
N, H, W, Q = args.frames, args.height, args.width, args.quality


def scene(n, h, w, c, rng, noise):
    """n frames: uniform noise, or a smooth moving pattern with discs and +-4 of noise (the clips of bench_mjpeg.py)"""
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
    from video.io.backend_mjpeg import VideoMJPEG, VideoWriterMJPEG
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

    def subsampled():
        try:
            from PIL import Image
        except ImportError:
            print("the subsampled leg needs Pillow to write its streams: skipped", flush=True)
            emit({"leg": "subsampled", "ms_per_call_median": "not measured", "note": "Pillow is not installed"})
            return
        pictures = scene(min(args.distinct, N), H, W, 3, np.random.default_rng(44), False)
        raw = N * H * W * 3
        out = torch.empty(raw, dtype=torch.uint8, device=dev)
        status = torch.zeros(N, dtype=torch.int32, device=dev)
        for restarts, kw in (("mcu_rows", {"restart_marker_rows": 1}), ("none", {})):
            for layout, sub in (("444", 0), ("422", 1), ("420", 2)):
                files = []
                for picture in pictures:
                    buf = io.BytesIO()
                    Image.fromarray(picture).save(buf, "JPEG", quality=Q, subsampling=sub, **kw)
                    files.append(buf.getvalue())
                files = [files[k % len(files)] for k in range(N)]
                heads = [ops.jpeg_parse_header(f, sampling="any") for f in files[:len(pictures)]]
                head = heads[0]
                assert len(ops.jpeg_decode_groups(heads)) == 1
                lh, lv = head["sampling"]
                ri = head["ri"]
                tables = b"".join(ops._jpeg_decode_table(*dc) + ops._jpeg_decode_table(*ac) for dc, ac in head["huff"])
                consts = torch.from_numpy(np.frombuffer(head["qtables"].tobytes() + tables, np.uint8).copy()).to(dev)
                src = torch.from_numpy(np.frombuffer(b"".join(files), np.uint8).copy()).to(dev)
                offsets = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)
                scans = np.array([heads[k % len(heads)]["scan_begin"] for k in range(N)], np.int64)
                meta = torch.from_numpy(np.concatenate([offsets, scans])).to(dev)
                room = int(L.va_jpeg_decode_sampled_workspace_bytes(N, H, W, 3, ri, lh, lv))
                ws = torch.empty(room, dtype=torch.uint8, device=dev)
                # as ops.jpeg_decode chooses: the plain entry for 1 x 1, the _sampled one with (luma_h, luma_v) else
                entry, luma = ((L.va_jpeg_decode_u8, ()) if (lh, lv) == (1, 1) else
                               (L.va_jpeg_decode_sampled_u8, (lh, lv)))
                call = ((src.data_ptr(), meta.data_ptr(), meta.data_ptr() + 8 * (N + 1), N, H, W, 3, ri) + luma
                        + (consts.data_ptr(), consts.data_ptr() + 192, len(tables), out.data_ptr(), status.data_ptr(),
                           ws.data_ptr(), room, S))

                def decode():
                    check(entry(*call))
                reps, args.reps = args.reps, args.reps if restarts != "none" else min(args.reps, 3)
                try:
                    best, med = events(decode)
                finally:
                    args.reps = reps
                assert not bool(status.any())
                emit({"leg": "subsampled/%s/%s" % (layout, restarts), "frames": N, "h": H, "w": W, "quality": Q,
                      "distinct_pictures": len(pictures), "ms_per_call_min": round(best, 4),
                      "ms_per_call_median": round(med, 4), "frames_per_s": round(N / med * 1e3, 1),
                      "output_gb_per_s": round(raw / med / 1e6, 1), "bytes_in_per_frame": int(offsets[-1]) // N,
                      "restart_interval_mcus": ri, "segments_per_call": N * head["nseg"],
                      "blocks_per_segment": ri * (lh * lv + 2), "workspace_bytes": room,
                      "note": "Pillow-written; locate + entropy + %s, one chunk"
                              % ("reconstruct" if (lh, lv) == (1, 1) else "chroma planes + pixels")})
                del src, ws
    def split():
        try:
            from PIL import Image
        except ImportError:
            print("the split leg needs Pillow to write its streams: skipped", flush=True)
            emit({"leg": "split", "ms_per_call_median": "not measured", "note": "Pillow is not installed"})
            return

        def prepare(pictures, n, sub, rows):
            """n Pillow-written files of one header, resident on the device, and what both entries need"""
            files = []
            for picture in pictures:
                buf = io.BytesIO()
                Image.fromarray(picture).save(buf, "JPEG", quality=Q, subsampling=sub,
                                              **({"restart_marker_rows": 1} if rows else {}))
                files.append(buf.getvalue())
            files = [files[k % len(files)] for k in range(n)]
            heads = [ops.jpeg_parse_header(f, sampling="any") for f in files[:len(pictures)]]
            assert len(ops.jpeg_decode_groups(heads)) == 1 and (rows or heads[0]["nseg"] == 1)
            head = heads[0]
            tables = b"".join(ops._jpeg_decode_table(*dc) + ops._jpeg_decode_table(*ac) for dc, ac in head["huff"])
            offsets = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)
            scans = np.array([heads[k % len(heads)]["scan_begin"] for k in range(n)], np.int64)
            return dict(head=head, tables=tables, n=n, offsets=offsets, scan_bytes=np.diff(offsets) - scans,
                        consts=torch.from_numpy(np.frombuffer(head["qtables"].tobytes() + tables, np.uint8).copy()).to(dev),
                        src=torch.from_numpy(np.frombuffer(b"".join(files), np.uint8).copy()).to(dev),
                        meta=torch.from_numpy(np.concatenate([offsets, scans])).to(dev))

        def timed(w, n, h, wd, sub_bytes=None, max_rounds=None, reps=None):
            """(min, median, rounds or None) of one call on the first n frames: the one-lane entry for sub_bytes None"""
            head = w["head"]
            lh, lv = head["sampling"]
            out = torch.empty(n * h * wd * 3, dtype=torch.uint8, device=dev)
            status = torch.zeros(n, dtype=torch.int32, device=dev)
            rounds = torch.zeros(n, dtype=torch.int32, device=dev)
            front = (w["src"].data_ptr(), w["meta"].data_ptr(), w["meta"].data_ptr() + 8 * (w["n"] + 1), n, h, wd, 3)
            mid = (w["consts"].data_ptr(), w["consts"].data_ptr() + 192, len(w["tables"]), out.data_ptr(), status.data_ptr())
            if sub_bytes is None:
                room = int(L.va_jpeg_decode_sampled_workspace_bytes(n, h, wd, 3, head["ri"], lh, lv))
                ws = torch.empty(room, dtype=torch.uint8, device=dev)
                call = lambda: check(L.va_jpeg_decode_sampled_u8(*(front + (head["ri"], lh, lv) + mid
                                                                  + (ws.data_ptr(), room, S))))
            else:
                most = int(w["scan_bytes"][:n].max())
                room = int(L.va_jpeg_decode_split_workspace_bytes(n, h, wd, 3, lh, lv, sub_bytes, most))
                ws = torch.empty(room, dtype=torch.uint8, device=dev)
                call = lambda: check(L.va_jpeg_decode_split_u8(*(front + (lh, lv) + mid + (
                    ws.data_ptr(), room, sub_bytes, max_rounds, most, rounds.data_ptr(), S))))
            keep, args.reps = args.reps, reps or args.reps
            try:
                best, med = events(call)
            finally:
                args.reps = keep
            assert not bool(status.any())
            return round(best, 4), round(med, 4), (None if sub_bytes is None else rounds.cpu().numpy())

        def rounds_row(r):
            return {"rounds_max": int(r.max()), "rounds_mean": round(float(r[r >= 0].mean()), 2) if (r >= 0).any() else None,
                    "frames_fallen_back": int((r < 0).sum())}
        pictures = scene(min(args.distinct, N), H, W, 3, np.random.default_rng(44), False)
        sub0, rounds0 = ops.JPEG_SPLIT_SUB_BYTES, ops.JPEG_SPLIT_MAX_ROUNDS
        for layout, sub in (("444", 0), ("422", 1), ("420", 2)):
            w = prepare(pictures, N, sub, False)
            base = {"frames": N, "h": H, "w": W, "quality": Q, "entropy_bytes_per_frame": int(w["scan_bytes"].mean())}
            if args.split_brief:
                timed(w, N, H, W, sub0, rounds0, reps=2)
                continue
            for n in sorted({min(32, N), N}):
                _, one_lane, _ = timed(w, n, H, W, reps=3)
                best, med, r = timed(w, n, H, W, sub0, rounds0)
                row = dict(base, leg="split/%s/none" % layout, frames=n, one_lane_ms_median=one_lane,
                           split_ms_min=best, split_ms_median=med, speedup=round(one_lane / med, 1),
                           frames_per_s=round(n / med * 1e3, 1), sub_bytes=sub0, max_rounds=rounds0,
                           note="Pillow-written, no restart markers; one_lane is va_jpeg_decode_sampled_u8, the only "
                                "path before the split entry, in the same run")
                row.update(rounds_row(r))
                emit(row)
            for sub_bytes in (128, 256, 512, 1024):
                best, med, r = timed(w, N, H, W, sub_bytes, 16)
                emit(dict(base, leg="split_sweep/%s" % layout, sub_bytes=sub_bytes, max_rounds=16, split_ms_min=best,
                          split_ms_median=med, **rounds_row(r)))
            for most in (1, 2, 4, 8, 16):
                best, med, r = timed(w, N, H, W, sub0, most, reps=3)
                emit(dict(base, leg="split_rounds/%s" % layout, sub_bytes=sub0, max_rounds=most, split_ms_min=best,
                          split_ms_median=med, **rounds_row(r)))
            del w
            rows_w = prepare(pictures, N, sub, True)
            best, med, _ = timed(rows_w, N, H, W)
            emit(dict(base, leg="split/%s/mcu_rows" % layout, ms_per_call_min=best, ms_per_call_median=med,
                      note="the same pictures with a restart interval per MCU row, va_jpeg_decode_sampled_u8"))
            del rows_w
        if args.split_brief:
            return
        for side in (64, 128, 256, 512):
            small = scene(8, side, side, 3, np.random.default_rng(45), False)
            w = prepare(small, 32, 2, False)
            _, one_lane, _ = timed(w, 32, side, side)
            _, med, r = timed(w, 32, side, side, sub0, rounds0)
            emit(dict(leg="split_crossover/420", frames=32, h=side, w=side, quality=Q,
                      entropy_bytes_per_frame=int(w["scan_bytes"].mean()), one_lane_ms_median=one_lane,
                      split_ms_median=med, sub_bytes=sub0, max_rounds=rounds0, **rounds_row(r)))
            del w
    if "split" in LEGS:
        split()
        ops.pool_clear()
    if "subsampled" in LEGS:
        subsampled()
        ops.pool_clear()
    for c in [m for m in (1, 3) if ("rgb" if m == 3 else "mono") in args.modes.split(",")]:
        for noise in (False, True):
            name = "%s/%s" % ("rgb" if c == 3 else "mono", "noise" if noise else "smooth")
            if not LEGS & {"kernels", "batch32", "ops", "pillow", "video"}:
                continue
            clip = scene(N, H, W, c, rng, noise)
            raw = clip.nbytes
            stack = ops.DeviceFrames.upload(clip)
            blob, offsets = ops.jpeg_encode(stack, Q, ret_packed=True)
            stack.release()
            ops.pool_clear()
            head = ops.jpeg_parse_header(blob[:offsets[1]].tobytes())
            ri = head["ri"]
            if LEGS & {"kernels", "batch32"}:
                tables = b"".join(ops._jpeg_decode_table(*dc) + ops._jpeg_decode_table(*ac) for dc, ac in head["huff"])
                consts = torch.from_numpy(np.frombuffer(head["qtables"].tobytes() + tables, np.uint8).copy()).to(dev)
                src = torch.from_numpy(blob).to(dev)
                meta = torch.from_numpy(np.concatenate([offsets, np.full(N, head["scan_begin"], np.int64)])).to(dev)
                out = torch.empty(raw, dtype=torch.uint8, device=dev)
                status = torch.zeros(N, dtype=torch.int32, device=dev)
                room = int(L.va_jpeg_decode_workspace_bytes(N, H, W, c, ri))
                ws = torch.empty(room, dtype=torch.uint8, device=dev)

                def decode(n):
                    check(L.va_jpeg_decode_u8(src.data_ptr(), meta.data_ptr(), meta.data_ptr() + 8 * (N + 1), n, H, W,
                                              c, ri, consts.data_ptr(), consts.data_ptr() + 64 * c, len(tables),
                                              out.data_ptr(), status.data_ptr(), ws.data_ptr(), room, S))
                if "kernels" in LEGS:
                    best, med = events(lambda: decode(N))
                    assert not bool(status.any())
                    twin = torch.empty_like(out)
                    _, copy_med = events(lambda: twin.copy_(out))
                    del twin
                    frames = torch.from_numpy(clip).to(dev)
                    ehead = np.frombuffer(ops.jpeg_header(H, W, c, Q), np.uint8)
                    econsts = torch.from_numpy(np.concatenate(ops.jpeg_tables(Q) + (ehead,))).to(dev)
                    info = torch.zeros(2 * N + 2, dtype=torch.int64, device=dev)
                    cap = raw + N * 4096
                    eout = torch.empty(cap, dtype=torch.uint8, device=dev)
                    _, enc_med = events(lambda: check(L.va_jpeg_encode_u8(
                        frames.data_ptr(), N, H, W, c, econsts.data_ptr(), econsts.data_ptr() + 128, len(ehead),
                        info.data_ptr() + 16 + 8 * N, info.data_ptr() + 8, info.data_ptr(), eout.data_ptr(), cap, S)))
                    del frames, eout
                    emit({"leg": "kernels/" + name, "frames": N, "h": H, "w": W, "quality": Q,
                          "ms_per_call_min": round(best, 4), "ms_per_call_median": round(med, 4),
                          "frames_per_s": round(N / med * 1e3, 1), "output_gb_per_s": round(raw / med / 1e6, 1),
                          "bytes_in_per_frame": int(len(blob)) // N, "segments_per_call": N * head["nseg"],
                          "workspace_bytes": room, "memcpy_same_output_ms_median": round(copy_med, 4),
                          "times_the_memcpy": round(med / copy_med, 2), "encode_same_frames_ms_median": round(enc_med, 4),
                          "note": "locate + entropy + reconstruct, one chunk"})
                if "batch32" in LEGS:
                    best, med = events(lambda: decode(min(32, N)))
                    emit({"leg": "batch32/" + name, "frames": min(32, N), "ms_per_call_min": round(best, 4),
                          "ms_per_call_median": round(med, 4), "frames_per_s": round(min(32, N) / med * 1e3, 1),
                          "segments_per_call": min(32, N) * head["nseg"], "waves_of_the_entropy_launch":
                          -(-min(32, N) * head["nseg"] // 64), "note": "one lane per segment"})
                del src, out, ws
            if "ops" in LEGS:
                full = wall(lambda: ops.jpeg_decode((blob, offsets)), args.reps)

                def kept():
                    ops.jpeg_decode((blob, offsets), keep=True).release()
                keep = wall(kept, args.reps)

                def upload():
                    ops.DeviceFrames.upload(clip).release()
                    torch.cuda.synchronize()
                up = wall(upload, args.reps)
                emit({"leg": "ops/" + name, "frames": N, "h": H, "w": W, "quality": Q,
                      "jpeg_decode_with_upload_and_download_ms_median": round(full, 2),
                      "jpeg_decode_keep_with_upload_ms_median": round(keep, 2), "raw_upload_ms_median": round(up, 2),
                      "bytes_uploaded": int(len(blob)), "raw_bytes": raw,
                      "keep_frames_per_s": round(N / keep * 1e3, 1),
                      "note": "wall clock from pageable host memory; header parse on the host included"})
            if "pillow" in LEGS:
                row = {"leg": "pillow/" + name, "frames": args.cpu_frames, "quality": Q}
                try:
                    from PIL import Image
                except ImportError:
                    Image = None
                if Image is None or not args.cpu_frames:
                    row["ms_per_frame"] = "not measured"
                else:
                    t0 = time.perf_counter()
                    for k in range(args.cpu_frames):
                        np.asarray(Image.open(io.BytesIO(blob[offsets[k]:offsets[k + 1]].tobytes())))
                    row.update({"ms_per_frame": round((time.perf_counter() - t0) * 1e3 / args.cpu_frames, 2),
                                "note": "libjpeg through Pillow, one core"})
                emit(row)
            if "video" in LEGS:
                nv = min(args.video_frames, N)
                with tempfile.TemporaryDirectory() as tmp:
                    path = os.path.join(tmp, "bench.avi")
                    with VideoWriterMJPEG(path, size=(W, H), fps=25, is_color=c == 3, quality=Q) as writer:
                        for f in clip[:nv]:
                            writer.write_frame(f)

                    def iterate(decoder):
                        with VideoMJPEG(path, {"decoder": decoder}) as video:
                            return sum(int(f[0, 0].sum()) for f in video)
                    device = wall(lambda: iterate("device"), 3)
                    try:
                        import PIL  # noqa: F401
                        pillow = round(wall(lambda: iterate("pillow"), 1), 1)
                    except ImportError:
                        pillow = "not measured"
                emit({"leg": "video/" + name, "frames": nv, "device_decoder_ms_median": round(device, 1),
                      "device_decoder_frames_per_s": round(nv / device * 1e3, 1), "pillow_decoder_ms": pillow,
                      "note": "VideoMJPEG iteration, wall clock: file reads, header parses, upload, decode, download "
                              "and a copy per frame"})
            del clip, blob
            ops.pool_clear()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


main()
