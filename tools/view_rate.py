#!/usr/bin/env python3
"""What side views and wireframe cost in the ragged overlay launch (dyb_render_meshes_var_opt), event-timed on one stream.

32 people over 1920 x 1080 frames, meshes with SMPL's counts (6890 vertices, 13 776 faces): the ellipsoid of tools/render_times.py,
or --soup (the synthetic SMPL's random-triple faces, hundreds deep at every pixel - the stress case).  Four legs, as
``--save_res 1`` issues them with and without ``--side_view 270`` / ``--wireframe 1``:

  overlays            32 descriptors: every mesh over its frame (the plain entry's work: opts NULL)
  overlays+sides      64 descriptors: the 32 overlays, and the 32 meshes turned by 270 degrees about Y over white canvases
  overlays wire       the first leg as wireframe
  overlays+sides wire the second leg as wireframe

Buffers are made beforehand and the legs go through the C entry, so the figures are launches and kernels (for the legs with side
views also the host check of the matrices: one small copy and a wait for the stream per call), not allocations.  Before a leg is
timed its pictures are compared with ``Renderer.render`` of each mesh alone: equal bytes, or the tool stops.  One JSON line.

usage:  timeout 600 python tools/view_rate.py [--reps 20] [--soup]
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
from dynaboa_amd.render import RenderDesc, RenderOpts, Renderer, side_view_matrix           # noqa: E402
from render_times import timed, uv_ellipsoid                                                # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--soup", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    if a.soup:
        t = assets.make_synthetic_smpl(0)
        v, f = t["v_template"].astype(np.float32), t["faces"]
        v = v / np.abs(v[:, :2]).max() * 0.85
    else:
        v, f = uv_ellipsoid()
    P, H, W = 32, 1080, 1920
    V = len(v)
    verts = torch.from_numpy(np.stack([v * s for s in rng.uniform(0.8, 1.0, P)]).astype(np.float32)).to(dev)
    # a person about 600 px tall somewhere in the frame: scale = 600 / (W, H), the shift keeps the box inside
    cam1 = np.stack([np.full(P, 600.0 / W), np.full(P, 600.0 / H), rng.uniform(-1.5, 1.5, P), rng.uniform(-0.5, 0.5, P)], 1).astype(np.float32)
    frames = torch.from_numpy(rng.integers(0, 256, (P, H, W, 3), dtype=np.uint8)).to(dev)
    white = torch.full((H, W, 3), 255, dtype=torch.uint8, device=dev)
    side = side_view_matrix(270.0, [0, 1, 0])
    lib = _lib.load()
    out = dict(what=f"{P} people ({'soup' if a.soup else 'ellipsoid'}, {len(f)} faces) over {W}x{H}", reps=a.reps)
    for wire in (0, 1):
        r = Renderer(resolution=(W, H), faces=f, device=dev, wire=bool(wire))
        faces, ptr, idx = r._adjacency(V, dev)
        F = int(faces.shape[0])
        want_front = [r.render(frames[i], verts[i], torch.from_numpy(cam1[i]).to(dev)) for i in range(P)]
        want_side = [r.render(white, verts[i], torch.from_numpy(cam1[i]).to(dev), angle=270, axis=[0, 1, 0]) for i in range(P)]
        for sides in (0, 1):
            N = P * (1 + sides)
            outs = [torch.empty(H, W, 3, dtype=torch.uint8, device=dev) for _ in range(N)]
            # the order overlay_jobs gives: a person's overlay, then the side view
            who = [i // (1 + sides) for i in range(N)]
            is_side = [bool(sides and i % 2) for i in range(N)]
            desc = (RenderDesc * N)(*[RenderDesc(verts[who[i]].data_ptr(), (white if is_side[i] else frames[who[i]]).data_ptr(), outs[i].data_ptr(), H, W)
                                      for i in range(N)])
            cam = torch.from_numpy(cam1[who]).to(dev).contiguous()
            model = torch.from_numpy(np.stack([side if s else np.eye(3, dtype=np.float32) for s in is_side]).reshape(N, 9)).to(dev) if sides else None
            opts = RenderOpts(model.data_ptr() if sides else None, wire)
            nbytes = int(lib.dyb_render_var_workspace_bytes(N, V, F)) + (int(lib.dyb_render_model_workspace_bytes(N, V)) if sides else 0)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

            def call():
                check(lib.dyb_render_meshes_var_opt(ctypes.cast(desc, ctypes.c_void_p), faces.data_ptr(), ptr.data_ptr(), idx.data_ptr(),
                                                    cam.data_ptr(), 1.0, 1.0, 0.9, N, V, F, 0, ws.data_ptr(), ws.numel(), stream_of(cam),
                                                    ctypes.addressof(opts) if (sides or wire) else None), "dyb_render_meshes_var_opt")
            call()
            torch.cuda.synchronize()
            for i in range(N):
                if not torch.equal(outs[i], (want_side if is_side[i] else want_front)[who[i]]):
                    raise SystemExit(f"picture {i} of the leg sides={sides} wire={wire} differs from the mesh drawn alone")
            p50, lo = timed(call, a.reps)
            name = ("overlays+sides" if sides else "overlays") + (" wire" if wire else "")
            drawn = float(np.mean([float((o != (white if s else frames[w])).any(-1).float().mean()) for o, s, w in zip(outs, is_side, who)]))
            out[name] = dict(descriptors=N, ms_median=round(p50, 3), ms_min=round(lo, 3), drawn_fraction=round(drawn, 4))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
