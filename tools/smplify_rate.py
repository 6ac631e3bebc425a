#!/usr/bin/env python3
"""Time per SMPLify fit at the reference's defaults (num_iters = 100 per stage, step size 1e-2) at B = 1, 8 and 66: the one-call
native loop (dyb_smplify_fit) against the autograd composition (``SMPLify(native=False)``: SMPL module + the two loss functions +
torch.optim.Adam) in the same process.

Inputs: the seeded samples of tests/golden/g12_smplify_fit.npz tiled to B, every copy's initial values moved by its own seeded noise;
the synthetic SMPL tables.  Method: both legs are warmed up (one full fit each), then timed in alternating rounds (native,
composition, native, ...), a host clock around a fit that ends in a device synchronise; per leg the median, the smallest and the
largest round are reported.  Before timing, the two legs' results are compared (they run the same iterations).  With
``--count-launches`` the kernel launches of one iteration of each stage are counted afterwards with torch.profiler, as the difference
between a 2-iteration and a 1-iteration fit.  No threshold: the figures are written down, nothing is asserted about them.

usage:  timeout 900 python tools/smplify_rate.py [--rounds 7] [--iters 100] [--batches 1,8,66] [--out profiles/r17_smplify.txt]
        timeout 300 python tools/smplify_rate.py --batches "" --count-launches        (the count alone, in a run of its own)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dynaboa_amd import assets                                                              # noqa: E402
from dynaboa_amd.smpl import SMPL                                                           # noqa: E402
from dynaboa_amd.smplify import SMPLify                                                     # noqa: E402


def inputs(B, dev):
    g = np.load(os.path.join(ROOT, "tests", "golden", "g12_smplify_fit.npz"))
    gen = torch.Generator().manual_seed(B)
    rep = lambda k: torch.from_numpy(g[k]).repeat((B + 2) // 3, *([1] * (g[k].ndim - 1)))[:B]
    x = {k: rep(k) for k in ("init_pose", "init_betas", "init_cam_t", "center", "kp")}
    x["init_pose"] = x["init_pose"] + 0.05 * torch.randn(B, 72, generator=gen)
    x["init_betas"] = x["init_betas"] + 0.1 * torch.randn(B, 10, generator=gen)
    x["init_cam_t"] = x["init_cam_t"] + torch.randn(B, 3, generator=gen) * torch.tensor([0.02, 0.02, 1.0])
    return [x[k].to(dev) for k in ("init_pose", "init_betas", "init_cam_t", "center", "kp")]


def fit_ms(f, x):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = f(*x)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def count_launches(f, x):
    """Kernel launches per iteration of (stage 1 + stage 2): a 2-iteration fit minus a 1-iteration fit."""
    from torch.profiler import ProfilerActivity, profile
    n = {}
    for it in (1, 2):
        f(*x, num_iters=it)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            f(*x, num_iters=it)
            torch.cuda.synchronize()
        n[it] = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
                    and "memset" not in e.name.lower())
    return n[2] - n[1]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--batches", default="1,8,66")
    ap.add_argument("--out", default=None)
    ap.add_argument("--count-launches", action="store_true")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("smplify_rate measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    smpl = SMPL(tables=assets.make_synthetic_smpl(0))
    legs = {name: SMPLify(num_iters=a.iters, device=dev, smpl=smpl, native=native) for name, native in (("native", True), ("composition", False))}
    lines = [f"SMPLify fit, {a.iters} iterations per stage, step size 1e-2, {a.rounds} alternating rounds after one warm-up fit per leg; ms per fit"]
    res = {}
    for B in [int(b) for b in a.batches.split(",") if b]:
        x = inputs(B, dev)
        warm = {name: fit_ms(f, x)[1] for name, f in legs.items()}
        dev_pose = float((warm["native"][2] - warm["composition"][2]).abs().max())
        dev_verts = float((warm["native"][0] - warm["composition"][0]).abs().max())
        ms = {name: [] for name in legs}
        for _ in range(a.rounds):
            for name, f in legs.items():
                ms[name].append(fit_ms(f, x)[0])
        r = {name: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for name, v in ms.items()}
        r["speedup_of_medians"] = r["composition"]["median"] / r["native"]["median"]
        r["legs_differ"] = dict(pose=dev_pose, vertices=dev_verts)
        res[B] = r
        lines.append(f"B = {B:3d}   native {r['native']['median']:9.2f} (min {r['native']['min']:.2f}, max {r['native']['max']:.2f})   "
                     f"composition {r['composition']['median']:9.2f} (min {r['composition']['min']:.2f}, max {r['composition']['max']:.2f})   "
                     f"ratio of medians {r['speedup_of_medians']:.2f}   per iteration: native {r['native']['median'] / (2 * a.iters) * 1e3:.1f} us, "
                     f"composition {r['composition']['median'] / (2 * a.iters) * 1e3:.1f} us   "
                     f"legs differ by: pose {dev_pose:.2e}, vertices {dev_verts:.2e}")
        print(lines[-1], flush=True)
        if a.out:
            open(a.out, "w").write("\n".join(lines) + "\n")
    if a.count_launches:
        x = inputs(8, dev)
        for name, f in legs.items():
            n = count_launches(f, x)
            res.setdefault("launches_per_iteration_pair", {})[name] = n
            lines.append(f"kernel launches of one stage-1 iteration plus one stage-2 iteration (torch.profiler, B = 8): {name} {n}")
            print(lines[-1], flush=True)
            if a.out:
                open(a.out, "w").write("\n".join(lines) + "\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
