#!/usr/bin/env python3
"""One scene call (dyb_render_scenes: all people of a frame in one pass) against the chain of N uniform calls it replaces
(dyb_render_meshes, the picture of one call the frame of the next), event-timed on one stream.

Shapes: 2 / 8 / 32 people over 1280 x 720 and over 1920 x 1080, standing side by side in boxes of 0.6 frame heights whose
neighbours overlap (a quarter of a box apart, closer where the row would leave the frame; from 8 people on in two staggered
rows).  Meshes with SMPL's counts (6890 vertices, 13 776 faces): the
ellipsoid of tools/render_times.py (a closed surface with small faces, as a body is) and the synthetic SMPL of tests'
``smpl_case`` (faces = random vertex triples, hundreds deep at every pixel: the stress case).  Both legs go through the C entries
with buffers made beforehand, so the comparison is launches and kernels, not allocations.  Before a shape is timed the two pictures
are compared: equal bytes, or the tool stops.  Per shape: warm-up, then --rounds alternations of (--reps scene calls, --reps chains),
each window between two events; the figure is the least mean over the rounds, all rounds are printed.  One JSON line per shape.

usage:  timeout 600 python tools/scene_rate.py [--reps 30] [--rounds 3] [--people 2 8 32] [--mesh ellipsoid soup]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dynaboa_amd import _lib, assets                                                        # noqa: E402
from dynaboa_amd._abi import check                                                          # noqa: E402
from dynaboa_amd.hmr import stream_of                                                       # noqa: E402
from dynaboa_amd.render import RenderScene, convert_crop_cam_to_orig_img, track_color, vertex_face_csr      # noqa: E402
from render_times import uv_ellipsoid                                                       # noqa: E402


def people(n, W, H, rng):
    """-> (scale per person (n,), frame cameras (n, 4)): boxes of 0.6 H, centres spread over the frame width so that neighbours
    overlap; two staggered rows from 8 people on."""
    h = 0.6 * H
    per_row = n if n < 8 else n // 2
    step = min(0.25 * h, 0.8 * W / max(per_row - 1, 1))         # a person is about 0.29 h wide: neighbours overlap
    cx = 0.5 * W + step * (np.arange(per_row) - 0.5 * (per_row - 1))
    cx = np.concatenate([cx, cx + 0.5 * step])[:n] if n >= 8 else cx
    cy = np.array([0.5 * H if n < 8 else (0.4 * H if i < per_row else 0.6 * H) for i in range(n)])
    crop = np.stack([rng.uniform(0.8, 1.0, n), rng.uniform(-0.05, 0.05, n), rng.uniform(-0.05, 0.05, n)], 1)
    cam = convert_crop_cam_to_orig_img(crop, np.stack([cx, cy, np.full(n, h)], 1), W, H)
    return rng.uniform(0.85, 1.0, n), cam.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--people", type=int, nargs="+", default=[2, 8, 32])
    ap.add_argument("--mesh", nargs="+", default=["ellipsoid", "soup"], choices=["ellipsoid", "soup"])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    soup = assets.make_synthetic_smpl(0)
    meshes = {"ellipsoid": uv_ellipsoid(), "soup": (soup["v_template"].astype(np.float32) / np.abs(soup["v_template"][:, :2]).max() * 0.85, soup["faces"])}
    for kind in a.mesh:
        v0, f = meshes[kind]
        V, F = len(v0), len(f)
        ptr, idx = vertex_face_csr(f, V)
        faces, ptr, idx = (torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(dev) for x in (f, ptr, idx))
        for (W, H) in ((1280, 720), (1920, 1080)):
            for n in a.people:
                rng = np.random.default_rng(1000 * n + W)
                scale, cam_h = people(n, W, H, rng)
                verts = torch.from_numpy(np.stack([v0 * s for s in scale]).astype(np.float32)).to(dev)
                verts[:, :, 2] += 3.0
                cam = torch.from_numpy(cam_h).to(dev)
                cols_h = [track_color(i) for i in range(n)]
                cols = torch.tensor(cols_h, dtype=torch.float32, device=dev)
                frame = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
                out_s = torch.empty_like(frame)
                ping = [torch.empty_like(frame), torch.empty_like(frame)]
                ws_s = torch.empty(int(lib.dyb_render_scenes_workspace_bytes(n, V, F)), dtype=torch.uint8, device=dev)
                ws_u = torch.empty(int(lib.dyb_render_workspace_bytes(1, V, F)), dtype=torch.uint8, device=dev)
                st = stream_of(frame)
                desc = (RenderScene * 1)(RenderScene(frame.data_ptr(), out_s.data_ptr(), None, None, H, W, 0, n))
                vp = (ctypes.c_void_p * n)(*[verts[i].data_ptr() for i in range(n)])
                ms = (ctypes.c_int * n)(*[0] * n)

                def scene():
                    check(lib.dyb_render_scenes(ctypes.cast(desc, ctypes.c_void_p), 1, ctypes.cast(vp, ctypes.c_void_p), ctypes.cast(ms, ctypes.c_void_p),
                                                cam.data_ptr(), cols.data_ptr(), faces.data_ptr(), ptr.data_ptr(), idx.data_ptr(), n, V, F, 0,
                                                ws_s.data_ptr(), ws_s.numel(), st), "dyb_render_scenes")

                def chain():
                    src = frame
                    for i in range(n):
                        dst = ping[i & 1]
                        check(lib.dyb_render_meshes(verts[i].data_ptr(), faces.data_ptr(), ptr.data_ptr(), idx.data_ptr(), cam[i].data_ptr(),
                                                    src.data_ptr(), cols_h[i][0], cols_h[i][1], cols_h[i][2], dst.data_ptr(), None, None, 1, V, F, H, W,
                                                    ws_u.data_ptr(), ws_u.numel(), st), "dyb_render_meshes")
                        src = dst
                    return src

                scene()
                last = chain()
                torch.cuda.synchronize()
                if not torch.equal(out_s, last):
                    raise SystemExit(f"{kind} {W}x{H} n={n}: the scene call and the chain differ at {int((out_s != last).any(-1).sum())} pixels")
                drawn = float((out_s != frame).any(-1).float().mean())
                for _ in range(3):
                    scene(); chain()
                torch.cuda.synchronize()
                t_scene, t_chain = [], []
                for _ in range(a.rounds):
                    for fn, ts in ((scene, t_scene), (chain, t_chain)):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(a.reps):
                            fn()
                        e1.record()
                        torch.cuda.synchronize()
                        ts.append(round(e0.elapsed_time(e1) / a.reps, 4))
                print(json.dumps(dict(mesh=kind, frame=[H, W], people=n, drawn=round(drawn, 3), reps=a.reps, ms_scene=min(t_scene), ms_chain=min(t_chain),
                                      chain_over_scene=round(min(t_chain) / min(t_scene), 2), ms_scene_all=t_scene, ms_chain_all=t_chain,
                                      launches_scene=4, launches_chain=3 * n)), flush=True)


if __name__ == "__main__":
    main()
