"""tools/bench_jpeg_encode.py - the device JPEG encoder (datasets.jpeg.JpegEncoder / sp_jpeg_encode_batch) next to the two ways a frame
leaves the device without it: the raw copy, and the raw copy followed by PIL's encoder on 16 threads.

Frames are synthesised (smooth structure plus noise, seeded): 1920x1080 and 256x192, encoded at 4:2:0 quality 75 without restart markers
and with one restart interval per MCU row.  For each it reports, per batch of B frames,
  * device ms (HIP events around the launches of one batch, descriptor upload excluded), ms per frame, MB/s of source pixels, and the
    split over the four stages (each stage launched alone on the same batch);
  * `encode()` as the host sees it: plan + upload + launches + the copy of the files + one synchronise;
  * the copy of the raw frames to pinned host memory, and that copy followed by PIL's encode on 16 threads (when PIL is installed);
  * the copy of the encoded files alone (what crosses the bus instead of the raw frames), and the time JpegDecoder takes for the files;
  * whether the first file equals PIL's byte for byte (when PIL is installed).
Every time is [median, min, max] in ms over separately timed runs (--iters device runs, 7 wall-clock runs).  The parent process never
touches the GPU: every configuration runs in a child of its own under `timeout`, one at a time, and the first child that fails ends the
run.  Writes ONE JSON line (and --out, default profiles/jpeg_encode_bench.json).

    python tools/bench_jpeg_encode.py [--iters 10] [--out profiles/jpeg_encode_bench.json]
"""
from __future__ import annotations

import argparse
import io
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# name, width, height, frames per batch, restart interval (MCUs)
CONFIGS = [("1920x1080", 1920, 1080, 4, 0), ("1920x1080_rst", 1920, 1080, 4, 120), ("256x192", 256, 192, 64, 0), ("256x192_rst", 256, 192, 64, 16)]
THREADS = 16
REPS = 7


def make_frames(w, h, n, seed=0):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    out = []
    for _ in range(n):
        ch = []
        for _c in range(3):
            a, b, p, q = rng.uniform(-1, 1, 4)
            ch.append(128 + 60 * np.sin(p * 6 + xx * (0.01 + 0.03 * abs(a))) * np.cos(q * 6 + yy * (0.01 + 0.03 * abs(b))) + rng.normal(0, 6, (h, w)))
        out.append(np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8))
    return np.stack(out)


def child(name, iters):
    import torch
    from simple_pose_amd import _lib
    from simple_pose_amd.datasets.jpeg import JpegDecoder, JpegEncoder
    try:
        from PIL import Image
    except ImportError:
        Image = None
    _, w, h, B, restart = next(c for c in CONFIGS if c[0] == name)
    host_frames = make_frames(w, h, B)
    frames = torch.from_numpy(host_frames).cuda()
    enc = JpegEncoder("cuda", quality=75, subsampling="4:2:0", restart_interval=restart)
    files = enc.encode(frames)
    res = {"frames": B, "restart_interval": restart, "file_kB_mean": round(float(np.mean([len(f) for f in files])) / 1e3, 1),
           "raw_kB": round(w * h * 3 / 1e3, 1)}

    def pil_one(i):
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(pinned_np[i][:, :, ::-1]), "RGB").save(buf, "JPEG", quality=75, subsampling=2, restart_marker_blocks=restart)
        return buf.getvalue()

    def spread(ms):
        return [round(float(np.median(ms)), 3), round(float(min(ms)), 3), round(float(max(ms)), 3)]

    def events(fn, n):
        fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for e0, e1 in ev:
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        return spread([e0.elapsed_time(e1) for e0, e1 in ev])

    def wall(fn, n):
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return spread(out)

    enc.encode_device(frames)
    ms = events(enc.relaunch, iters)
    res["device_ms"] = ms
    res["device_ms_per_frame"] = round(ms[0] / B, 4)
    res["device_source_MB_s"] = round(B * w * h * 3 / ms[0] / 1e3, 1)
    res["stages_ms"] = {k: events(lambda s=s: enc.relaunch(s), iters) for k, s in
                        (("coef", _lib.SP_JPEG_ENC_STAGE_COEF), ("scan", _lib.SP_JPEG_ENC_STAGE_SCAN), ("emit", _lib.SP_JPEG_ENC_STAGE_EMIT),
                         ("stuff", _lib.SP_JPEG_ENC_STAGE_STUFF))}
    res["dominant_stage"] = max(res["stages_ms"], key=lambda k: res["stages_ms"][k][0])
    res["encode_call_ms"] = wall(lambda: enc.encode(frames), REPS)
    res["encode_call_ms_per_frame"] = round(res["encode_call_ms"][0] / B, 4)
    # the raw frames to pinned memory; the files alone (as one packed device buffer) to pinned memory
    pinned = torch.empty(frames.shape, dtype=torch.uint8).pin_memory()
    pinned_np = pinned.numpy()
    res["raw_copy_ms"] = wall(lambda: pinned.copy_(frames, non_blocking=True), REPS)
    packed = torch.from_numpy(np.frombuffer(b"".join(files), np.uint8).copy()).cuda()
    pinned_files = torch.empty(packed.shape, dtype=torch.uint8).pin_memory()
    res["files_copy_ms"] = wall(lambda: pinned_files.copy_(packed, non_blocking=True), REPS)
    res["encode_plus_files_copy_ms"] = [round(res["device_ms"][0] + res["files_copy_ms"][0], 3)]
    res["encode_call_vs_raw_copy"] = round(res["encode_call_ms"][0] / res["raw_copy_ms"][0], 2)
    if Image is not None:
        from concurrent.futures import ThreadPoolExecutor
        pool = ThreadPoolExecutor(THREADS)

        def raw_then_pil():
            pinned.copy_(frames, non_blocking=True)
            torch.cuda.synchronize()
            return list(pool.map(pil_one, range(B)))
        res["exact_vs_pil"] = bool(raw_then_pil()[0] == files[0])
        res[f"raw_copy_plus_pil_{THREADS}_threads_ms"] = wall(raw_then_pil, REPS)
    dec = JpegDecoder("cuda")
    dec.decode(files)
    res["decode_device_ms"] = events(dec.relaunch, iters)
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_encode_bench.json"))
    ap.add_argument("--step-timeout", type=int, default=150)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.iters)
        return 0
    res = {"bench": "jpeg_encode", "threads": THREADS, "times": "[median, min, max] ms per batch of `frames` frames",
           "frames_are": "4:2:0, quality 75; _rst = one restart interval per MCU row"}
    for name, *_ in CONFIGS:                                   # one GPU process at a time, each under its own timeout
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", name, "--iters", str(args.iters)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        line = next((l for l in r.stdout.splitlines() if l.startswith("RESULT ")), None)
        if r.returncode != 0 or line is None:
            res[name] = {"failed": r.returncode, "stderr": r.stderr[-800:]}
            print(json.dumps(res))
            return 1                                           # nothing more is started on the GPU after a failure
        res[name] = json.loads(line[7:])
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
