#!/usr/bin/env python3
"""Frames/s of ONE online sequence (dynaboa_amd.online.OnlineAdaptor, use_boa 1, dynamic_boa 0, the native stepper) on synthetic
frames: (i) crops and keypoints resident on the device - the adaptation alone; (ii) uint8 host frames uploaded, boxed and cropped
inside the clock - what a camera loop sees.  One process, a warm-up, then --frames frames per leg; prints one JSON line.

usage:  timeout 300 python tools/online_rate.py [--frames 200] [--warmup 20] [--interval 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dynaboa_amd import assets, online as ON                    # noqa: E402
from dynaboa_amd.base_adaptor import synthetic_bundle           # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--interval", type=int, default=5)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = dict(frames=a.frames, warmup=a.warmup, interval=a.interval, frame_size=[a.height, a.width])
    rng = np.random.default_rng(0)
    for leg in ("resident", "host_frames"):
        ad = ON.OnlineAdaptor(ON.online_options(use_boa=1, dynamic_boa=0, interval=a.interval), synthetic_bundle(seed=22, randomize_norm=True), device=dev)
        if leg == "resident":
            items = [{k: v.to(dev) for k, v in assets.make_online_frame(i).items()} for i in range(16)]
            step = lambda i: ad.adapt_processed(items[i % 16]["image"], items[i % 16]["smpl_j2d"])
        else:
            frames = [rng.integers(0, 255, (a.height, a.width, 3), dtype=np.uint8) for _ in range(8)]
            kps = [np.concatenate([rng.uniform([400, 100], [880, 620], (25, 2)), rng.uniform(0.2, 1.0, (25, 1))], 1).astype(np.float32) for _ in range(8)]
            step = lambda i: ad.online_adaptation(frames[i % 8], kps[i % 8])
        for i in range(a.warmup):
            step(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.frames):
            res = step(a.warmup + i)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert ad._native is not None and torch.isfinite(res["vts"]).all()
        out[leg] = dict(frames_per_s=round(a.frames / dt, 2), ms_per_frame=round(1e3 * dt / a.frames, 3))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
