"""tools/bench_augment.py - cost of the GPU training transform (RefineSimpleTransform.batch / GpuAugmentLoader).  Prints ONE JSON line:

  * device time per batch of sp_warp_affine_batch_u8c3_to_nchw_f32 (+ the refine encoder) from HIP events, after warm-up, B = 32 and 128,
    samples drawn from 640x480 sources;
  * host time per batch: the draws + matrices (`geometry`), and the whole `batch()` call as the host sees it (draws, matrices, uploads,
    launches; no synchronisation);
  * the CPU reference cost per sample for comparison: the C restatement of cv.warpAffine (oracle) + a numpy full-map Gaussian encoder;
  * the bf16 B = 32 ResNet50-DConv train step fed by GpuAugmentLoader against the same step fed by SyntheticLoader, alternated in one
    process (ms per step, loader time included).

    python tools/bench_augment.py [--steps 20] [--rounds 3] [--out profiles/augment_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from simple_pose_amd.commons.transforms import RefineSimpleTransform  # noqa: E402
from simple_pose_amd.datasets.coco import COCO_JOINT_PAIRS, GpuAugmentLoader  # noqa: E402


def make_samples(n, n_src=16, seed=0):
    rng = np.random.default_rng(seed)
    imgs = [torch.from_numpy(rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)).cuda() for _ in range(n_src)]
    out = []
    for i in range(n):
        x1, y1 = rng.uniform(0, 400), rng.uniform(0, 200)
        x2, y2 = x1 + rng.uniform(60, 230), y1 + rng.uniform(120, 270)
        j = np.zeros((17, 3), np.float32)
        j[:, 0], j[:, 1] = rng.uniform(x1, x2, 17), rng.uniform(y1, y2, 17)
        j[:, 2] = (rng.random(17) > 0.2).astype(np.float32)
        out.append(types.SimpleNamespace(img=imgs[i % n_src], box=[x1, y1, x2, y2], joints=j, shape=(640, 480), img_id=i))
    return out


def device_us(tf, samples, iters=50):
    rng = (__import__("random").Random(0), np.random.RandomState(0))
    for _ in range(5):
        tf.batch(samples, rng)
    torch.cuda.synchronize()
    # the kernel alone: the same matrices every launch (what the events bracket is GPU work only)
    geo = tf.geometry(samples, rng)
    from simple_pose_amd import _lib
    import ctypes
    n = len(samples)
    x = torch.empty((n, 3, 256, 192), device="cuda")
    srcs = np.array([s.img.data_ptr() for s in samples], np.uint64)
    hw = np.array([s.img.shape[:2] for s in samples], np.int32)
    mean = (ctypes.c_float * 3)(0.485, 0.456, 0.406)
    m = np.ascontiguousarray(geo.m_fwd)
    hmj = torch.from_numpy(geo.hm_joints).cuda()
    hm = torch.empty((n, 17, 64, 48), device="cuda")
    mk = torch.empty((n, 17), device="cuda")
    st = _lib.current_stream()
    lib = _lib.lib()

    def warp():
        _lib.check(lib.sp_warp_affine_batch_u8c3_to_nchw_f32(srcs.ctypes.data, hw.ctypes.data, geo.flip.ctypes.data, m.ctypes.data, n, 256, 192,
                                                              mean, _lib.ptr(x), None, st))

    def enc():
        _lib.check(lib.sp_encode_gauss_refine(_lib.ptr(hmj), n, 17, 64, 48, 2.0, _lib.ptr(hm), _lib.ptr(mk), st))

    res = {}
    for name, fn in (("warp", warp), ("encode", enc)):
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        res[name] = e0.elapsed_time(e1) * 1e3 / iters
    return res


def host_ms(tf, samples, iters=30):
    import random
    rng = (random.Random(1), np.random.RandomState(1))
    t0 = time.perf_counter()
    for _ in range(iters):
        tf.geometry(samples, rng)
    geo = (time.perf_counter() - t0) * 1e3 / iters
    torch.cuda.synchronize()
    tot = 0.0
    for _ in range(iters):
        t0 = time.perf_counter()
        tf.batch(samples, rng)
        tot += time.perf_counter() - t0
        torch.cuda.synchronize()
    return geo, tot * 1e3 / iters


def cpu_reference_ms_per_sample(samples, n=8):
    from oracle import pose_oracle
    tf = RefineSimpleTransform(COCO_JOINT_PAIRS)
    geo = tf.geometry(samples[:n])
    imgs = [s.img.cpu().numpy() for s in samples[:n]]
    yy, xx = np.meshgrid(np.arange(64), np.arange(48), indexing="ij")
    t0 = time.perf_counter()
    for i in range(n):
        src = np.fliplr(imgs[i]) if geo.flip[i] else imgs[i]
        pose_oracle.warp_affine_u8c3(src, geo.m_fwd[i], (192, 256))
    t_warp = (time.perf_counter() - t0) * 1e3 / n
    t0 = time.perf_counter()
    for i in range(n):                                  # numpy full-map Gaussian per joint, float64 then float32, as the reference's encoder
        tg = np.zeros((17, 64, 48), np.float32)
        for j, (mx, my, v) in enumerate(geo.hm_joints[i]):
            if v > 0.5:
                tg[j] = np.exp(-((xx - mx) ** 2 + (yy - my) ** 2) / 8.0)
    t_enc = (time.perf_counter() - t0) * 1e3 / n
    return t_warp, t_enc


def train_compare(steps, rounds, warmup=3):
    from simple_pose_amd.nets import pose_resnet_dconv
    from simple_pose_amd.processors.ddp_pose_resnet_solver import SyntheticLoader
    from simple_pose_amd.train import PoseTrainer
    B = 32
    torch.manual_seed(0)
    model = pose_resnet_dconv.resnet50(pretrained=False, num_classes=17).cuda().train()
    trainer = PoseTrainer(model, lr=1e-3, dtype="bf16")
    tpath = os.path.join(ROOT, "profiles", "r06_train_bf16_tiles.json")
    if os.path.isfile(tpath):
        with open(tpath) as fh:
            trainer.set_tiles(json.load(fh), B)
    gpu_loader = GpuAugmentLoader(make_samples(B * (steps + warmup), seed=3), B, 0, 1, seed=0)
    syn_loader = SyntheticLoader(B * (steps + warmup), B, 17, 0, 1, torch.device("cuda"))

    def run(loader):
        it = iter(loader)
        for _ in range(warmup):
            xb, hm, mk, _, _ = next(it)
            trainer.step(xb, hm, mk)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            xb, hm, mk, _, _ = next(it)
            trainer.step(xb, hm, mk)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    gpu, syn = [], []
    for r in range(rounds):
        gpu_loader.set_epoch(r)
        syn.append(run(syn_loader))
        gpu.append(run(gpu_loader))
    return gpu, syn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    tf = RefineSimpleTransform(COCO_JOINT_PAIRS)
    res = {"bench": "augment", "device": torch.cuda.get_device_name(0)}
    for B in (32, 128):
        samples = make_samples(B, seed=B)
        d = device_us(tf, samples)
        g, h = host_ms(tf, samples)
        res[f"B{B}"] = {"warp_us": round(d["warp"], 2), "encode_us": round(d["encode"], 2), "host_geometry_ms": round(g, 3),
                        "host_batch_call_ms": round(h, 3), "warp_bytes_written_MB": round(B * 256 * 192 * 12 / 1e6, 2)}
    tw, te = cpu_reference_ms_per_sample(make_samples(8, seed=5))
    res["cpu_reference_ms_per_sample"] = {"warp": round(tw, 3), "numpy_encode": round(te, 3), "sum": round(tw + te, 3)}
    if not args.no_train:
        gpu, syn = train_compare(args.steps, args.rounds)
        res["train_bf16_b32_ms"] = {"gpu_augment_loader": [round(v, 3) for v in gpu], "synthetic_loader": [round(v, 3) for v in syn],
                                    "ratio_median": round(float(np.median(gpu) / np.median(syn)), 4)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
