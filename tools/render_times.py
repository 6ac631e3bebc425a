#!/usr/bin/env python3
"""Time of the mesh overlay (csrc/render.hip) on two workloads, for a `rocprofv3 --kernel-trace --stats` run and by its own events:
  (a) 32 meshes at 224 x 224 in one launch (one per sequence of a 32-sequence step), (b) one mesh on a 1920 x 1080 frame.
The mesh is an ellipsoid with SMPL's counts (6890 vertices, 13 776 faces: a latitude / longitude sphere of 84 segments and 83 rings)
filling about the part of the crop a person does - a closed surface with small faces, as a body is.  The synthetic SMPL of
dynaboa_amd.assets (faces = random vertex triples, hundreds deep at every pixel) is a stress case, timed with `--soup`.
   python tools/render_times.py [--soup] [--reps 20]
   rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o render -- python tools/render_times.py"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch     # noqa: E402
from dynaboa_amd import assets     # noqa: E402
from dynaboa_amd.render import Renderer, convert_crop_cam_to_orig_img     # noqa: E402


def uv_ellipsoid(segments=84, rings=83, radii=(0.32, 0.85, 0.25)):
    th = np.pi * np.arange(1, rings) / rings
    ph = 2 * np.pi * np.arange(segments) / segments
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph)[None], np.cos(th)[:, None] * np.ones_like(ph)[None], np.sin(th)[:, None] * np.sin(ph)[None]], -1)
    v = np.concatenate([[[0, 1, 0]], ring.reshape(-1, 3), [[0, -1, 0]]]).astype(np.float64)
    idx = lambda r, s: 1 + r * segments + s % segments
    f = []
    for s in range(segments):
        f.append((0, idx(0, s), idx(0, s + 1)))
        f.append((len(v) - 1, idx(rings - 2, s + 1), idx(rings - 2, s)))
        for r in range(rings - 2):
            f.append((idx(r, s), idx(r + 1, s), idx(r + 1, s + 1)))
            f.append((idx(r, s), idx(r + 1, s + 1), idx(r, s + 1)))
    f = np.array(f, np.int64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    inward = (n * v[f].mean(1)).sum(1) < 0
    f[inward] = f[inward][:, ::-1]
    return (v * np.array(radii)).astype(np.float32), f


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--soup", action="store_true", help="the synthetic SMPL's random-triple faces instead of the ellipsoid")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    if a.soup:
        t = assets.make_synthetic_smpl(0)
        v, f = t["v_template"].astype(np.float32), t["faces"]
        v = v / np.abs(v[:, :2]).max() * 0.85
    else:
        v, f = uv_ellipsoid()
    print("mesh: %d vertices, %d faces (%s)" % (len(v), len(f), "random-triple soup" if a.soup else "ellipsoid"))
    # (a) 32 meshes, 224 x 224: each its own size, place and frame
    S = 32
    verts = torch.from_numpy(np.stack([v * s for s in rng.uniform(0.8, 1.0, S)]).astype(np.float32)).to(dev)
    cam = torch.from_numpy(np.concatenate([np.repeat(rng.uniform(0.8, 1.0, (S, 1)), 2, 1), rng.uniform(-0.1, 0.1, (S, 2))], 1).astype(np.float32)).to(dev)
    frames = torch.from_numpy(rng.integers(0, 256, (S, 224, 224, 3), dtype=np.uint8)).to(dev)
    r224 = Renderer(resolution=(224, 224), faces=f)
    out = r224.rasterize(verts, cam, frames)
    print("(a) 32 x 224 x 224: covered %.1f %% of the pixels" % (100.0 * float((out[1] >= 0).float().mean())))
    p50, lo = timed(lambda: r224.rasterize(verts, cam, frames), a.reps)
    print("(a) 32 x 224 x 224: %.3f ms per call (median of %d, min %.3f; three kernels)" % (p50, a.reps, lo))
    # (b) one mesh, 1920 x 1080, a 600 px box
    ocam = convert_crop_cam_to_orig_img(cam[:1, [0, 2, 3]], torch.tensor([[1000.0, 520.0, 600.0]], device=dev), 1920, 1080)
    frame = torch.from_numpy(rng.integers(0, 256, (1, 1080, 1920, 3), dtype=np.uint8)).to(dev)
    rhd = Renderer(resolution=(1920, 1080), faces=f)
    out = rhd.rasterize(verts[:1], ocam, frame)
    print("(b) 1 x 1920 x 1080: covered %.1f %% of the pixels" % (100.0 * float((out[1] >= 0).float().mean())))
    p50, lo = timed(lambda: rhd.rasterize(verts[:1], ocam, frame), a.reps)
    print("(b) 1 x 1920 x 1080: %.3f ms per call (median of %d, min %.3f)" % (p50, a.reps, lo))


if __name__ == "__main__":
    main()
