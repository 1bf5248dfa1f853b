#!/usr/bin/env python3
"""conv3 + next conv1 as one launch (sp_pw_chain_f32, `pwchain` ops) against the two launches, on the headline program (tools, not product):
per pair the median time of the launch(es) (a) alone, `--reps` back to back, and (b) in place, HIP events around them inside a one-stream forward;
plus the bytes the fused launch has to move and the TB/s that makes.  The unfused program runs with the tracked tile table bench.py uses.

    python tools/bench_pw_chain.py --batch 128 --out pw_chain_pairs.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import bench
    from simple_pose_amd import _lib, synth
    from simple_pose_amd.nets import pose_resnet_dconv

    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    model = pose_resnet_dconv.resnet50(pretrained=False, num_classes=17)
    sd = synth.conditioned_state_dict([(k, tuple(v.shape), str(v.dtype)) for k, v in model.state_dict().items()], seed=0)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model = model.to(dev).eval()
    B = args.batch
    x = torch.from_numpy(np.concatenate([synth.input_images(8, seed=100)] * ((B + 7) // 8), 0)[:B]).to(dev)
    tiles = bench.tracked_tiles("dconv", "f32")
    progs = {}
    for fused in (False, True):
        model.fuse_chain = fused
        prog = model.hip_program(x)
        prog.multi_stream = False
        if tiles:
            with open(tiles) as fh:
                prog.set_tiles(json.load(fh), B)
        prog.run(x)
        progs[fused] = prog
    torch.cuda.synchronize()
    stream = _lib.current_stream()

    def timed(prog, names, in_place):
        bufs = dict(prog._alloc(B, dev))
        bufs["input"] = x
        bufs[prog.out_name] = torch.empty((B,) + tuple(prog.out_shape), dtype=torch.float32, device=dev)
        sel = [op for op in prog.ops if op.name in names]
        assert len(sel) == len(names), (names, [op.name for op in sel])
        ts = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if in_place:
                for op in prog.ops:
                    if op is sel[0]:
                        e0.record()
                    prog._launch(lib, op, bufs, B, stream)
                    if op is sel[-1]:
                        e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3)
            else:
                e0.record()
                for _ in range(args.reps):
                    for op in sel:
                        prog._launch(lib, op, bufs, B, stream)
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) / args.reps * 1e3)
        torch.cuda.synchronize()
        return round(sorted(ts)[len(ts) // 2], 1)

    rows = []
    for a, c, c_next in (("layer1.1.conv3", "layer1.2.conv1", 64), ("layer1.2.conv3", "layer2.0.conv1", 128)):
        M = B * (x.shape[2] // 4) * (x.shape[3] // 4)
        mb = M * 4 * (64 + 256 + 256 + c_next) / 1e6
        row = {"pair": a + "+" + c, "rows": M, "fused_mb": round(mb, 1)}
        for key, in_place in (("alone", False), ("in_place", True)):
            two = timed(progs[False], (a, c), in_place)
            one = timed(progs[True], (a + "+" + c,), in_place)
            row[key] = {"two_launches_us": two, "fused_us": one, "fused_tb_per_s": round(mb / one, 2)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
