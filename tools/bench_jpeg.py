"""tools/bench_jpeg.py - throughput of the device JPEG decoder (datasets.jpeg.JpegDecoder / sp_jpeg_decode_batch) next to PIL on the same box.

Files are synthesised with PIL: 640x480 and 1280x720, 4:2:0, quality 90, without restart markers and with one per MCU row.  For 32, 128
and 512 files per call it reports
  * device ms per batch (HIP events around the launches, upload excluded) and img/s, and the split over the three kernels (each stage
    launched alone on the same batch; the entropy figure includes the launch that zeroes the coefficients);
  * `decode()` as the host sees it: parse + pinned upload + launches + one synchronise, ms per batch and img/s;
  * the baseline: PIL decode + upload of each image on 16 threads.
Every time is [median, min, max] in ms over separately timed runs (--iters device runs, 7 wall-clock runs); img/s is from the median.
The parent process never touches the GPU: every configuration runs in a child of its own under `timeout`, one at a time, and the first
child that fails ends the run.  Writes ONE JSON line (and --out, default profiles/jpeg_bench.json).
--progressive: the same for PIL's progressive saves of the 640x480 images (10 scans; sp_jpeg_progressive_entropy is the entropy stage),
written to profiles/jpeg_prog_bench.json.

    python tools/bench_jpeg.py [--progressive] [--iters 10] [--out profiles/jpeg_bench.json]
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

CONFIGS = [("640x480", 640, 480, False, False), ("640x480_rst", 640, 480, True, False), ("1280x720", 1280, 720, False, False),
           ("1280x720_rst", 1280, 720, True, False)]
PROGRESSIVE_CONFIGS = [("640x480_prog", 640, 480, False, True), ("640x480_prog_rst", 640, 480, True, True)]
BATCHES = (32, 128, 512)
THREADS = 16
DISTINCT = 16
REPS = 7                        # wall-clock repetitions of decode() and of the PIL baseline


def make_files(w, h, restart, progressive=False, n=DISTINCT, seed=0):
    from PIL import Image
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    files = []
    for _ in range(n):
        ch = []
        for _c in range(3):
            a, b, p, q = rng.uniform(-1, 1, 4)
            ch.append(128 + 60 * np.sin(p * 6 + xx * (0.01 + 0.03 * abs(a))) * np.cos(q * 6 + yy * (0.01 + 0.03 * abs(b))) + rng.normal(0, 6, (h, w)))
        buf = io.BytesIO()
        opts = dict(quality=90, subsampling=2)
        if restart:
            opts["restart_marker_rows"] = 1
        if progressive:
            opts["progressive"] = True
        Image.fromarray(np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8), "RGB").save(buf, "JPEG", **opts)
        files.append(buf.getvalue())
    return files


def child(name, iters):
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from simple_pose_amd import _lib
    from simple_pose_amd.datasets.jpeg import JpegDecoder
    _, w, h, restart, progressive = next(c for c in CONFIGS + PROGRESSIVE_CONFIGS if c[0] == name)
    distinct = make_files(w, h, restart, progressive)
    res = {"file_kB_mean": round(float(np.mean([len(f) for f in distinct])) / 1e3, 1)}
    dec = JpegDecoder("cuda")
    ref = np.asarray(Image.open(io.BytesIO(distinct[0])).convert("RGB"))[:, :, ::-1]
    res["exact_vs_pil"] = bool(np.array_equal(dec.decode(distinct[:1])[0].cpu().numpy(), ref))

    def events(fn, n):
        """[median, min, max] ms of n separately timed runs of fn (HIP events around each), after one warm-up run."""
        fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for e0, e1 in ev:
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        return spread([e0.elapsed_time(e1) for e0, e1 in ev])

    def spread(ms):
        return [round(float(np.median(ms)), 3), round(float(min(ms)), 3), round(float(max(ms)), 3)]

    def wall(fn, n):
        out = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return spread(out)

    def pil_one(data):
        return torch.from_numpy(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))).cuda(non_blocking=True)

    pool = ThreadPoolExecutor(THREADS)
    for B in BATCHES:
        files = [distinct[i % len(distinct)] for i in range(B)]
        dec.decode(files)
        ms = events(dec.relaunch, iters)
        split = {k: events(lambda s=s: dec.relaunch(s), iters) for k, s in
                 (("entropy", _lib.SP_JPEG_STAGE_ENTROPY), ("idct", _lib.SP_JPEG_STAGE_IDCT), ("color", _lib.SP_JPEG_STAGE_COLOR))}
        host_ms = wall(lambda: dec.decode(files), REPS)
        list(pool.map(pil_one, files[:THREADS]))
        torch.cuda.synchronize()
        pil_ms = wall(lambda: list(pool.map(pil_one, files)), REPS)
        res[f"B{B}"] = {"device_ms": ms, "device_img_s": round(B / ms[0] * 1e3, 1), "kernels_ms": split,
                        "decode_call_ms": host_ms, "decode_call_img_s": round(B / host_ms[0] * 1e3, 1),
                        f"pil_{THREADS}_threads_ms": pil_ms, f"pil_{THREADS}_threads_img_s": round(B / pil_ms[0] * 1e3, 1),
                        f"pil_{THREADS}_threads_img_s_best": round(B / pil_ms[1] * 1e3, 1)}
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--progressive", action="store_true", help="progressive files (PROGRESSIVE_CONFIGS) instead of baseline ones")
    ap.add_argument("--out", default=None, help="default: profiles/jpeg_bench.json, profiles/jpeg_prog_bench.json with --progressive")
    ap.add_argument("--step-timeout", type=int, default=150)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.iters)
        return 0
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "jpeg_prog_bench.json" if args.progressive else "jpeg_bench.json")
    res = {"bench": "jpeg_progressive" if args.progressive else "jpeg", "threads": THREADS, "times": "[median, min, max] ms",
           "files": "PIL, 4:2:0, quality 90; _rst = one restart marker per MCU row" + ("; _prog = progressive=True (10 scans)" if args.progressive else "")}
    for name, *_ in (PROGRESSIVE_CONFIGS if args.progressive else CONFIGS):                                   # one GPU process at a time, each under its own timeout
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
