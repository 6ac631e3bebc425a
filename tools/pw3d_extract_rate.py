#!/usr/bin/env python3
"""Rate of the 3DPW extraction on a synthetic set the size of the real test split: 24 sequences, 37 person-tracks (13 sequences with
two people, 11 with one), about 35k person-frames, 3 % of the frames without a valid camera pose; synthetic SMPL tables.

Two routes through the SAME host code (``pw3d_extract.extract_sequence``: masks, scatter, names, npz files), timed in alternating
rounds after one warm-up sequence each:
  device   this project's SMPL (csrc/smpl_lbs.hip) and ``dyb_pw3d_annotate`` on cuda:0, chunks of 1024 frames;
  host     the same arithmetic on the CPU: the oracle's LBS (oracle/ref_cpu.py, torch on --threads threads) in place of the SMPL module
           and, in place of ``annotate``, fp64 NumPy for projection and box plus the oracle's fp32 quaternion conversions for the
           root (``pw3d_extract.annotate`` is replaced for the duration of the host rounds; nothing else differs).
A host clock around the whole set; the device route ends in a device synchronise.  Reported per route: seconds for the set and
person-frames per second, median / smallest / largest round, and the largest deviation between the two routes' files.  Nothing is
asserted about the figures.

usage:  timeout 900 python tools/pw3d_extract_rate.py [--rounds 3] [--threads 16] [--out profiles/r19_pw3d_extract_rate.txt]
"""
import argparse
import json
import os
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dynaboa_amd import assets, pw3d_extract as PX                                          # noqa: E402
from dynaboa_amd.smpl import SMPL                                                           # noqa: E402
from oracle import ref_cpu as O                                                             # noqa: E402

PEOPLE = [2] * 13 + [1] * 11


def rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])}[axis]


def make_sequence(i, people):
    rng = np.random.default_rng(1000 + i)
    F = 560 + 37 * ((7 * i) % 24)
    walk = np.linspace(0.0, 1.0, F)
    cam_poses = np.tile(np.eye(4), (F, 1, 1))
    for f in range(F):
        R = rot("y", -0.3 + 0.6 * walk[f]) @ rot("x", np.pi - 0.1)
        cam_poses[f, :3, :3], cam_poses[f, :3, 3] = R, -R @ np.array([0.5 * walk[f], 1.1, 5.5])
    d = dict(poses=[], betas=[], trans=[], poses2d=[], campose_valid=[], genders=[], cam_poses=cam_poses,
             cam_intrinsics=np.array([[1961.85, 0.0, 540.0], [0.0, 1969.23, 960.0], [0.0, 0.0, 1.0]]), sequence=f"synthetic_{i:02d}",
             img_frame_ids=np.arange(F))
    for p in range(people):
        d["poses"].append(rng.standard_normal((F, 72)) * 0.25)
        d["betas"].append(rng.standard_normal(10) * 0.7)
        d["trans"].append(np.stack([-0.6 + 1.2 * p + 0.5 * walk, 0.9 + 0.0 * walk, 0.4 * walk], 1))
        d["poses2d"].append(rng.uniform(0.0, 1000.0, (F, 3, 18)))
        d["campose_valid"].append((rng.uniform(0, 1, F) > 0.03).astype(np.uint8))
        d["genders"].append("mf"[(i + p) % 2])
    return d


class HostSMPL:
    def __init__(self, tables):
        self.T = O.smpl_tables_to_torch(tables)

    def __call__(self, betas=None, body_pose=None, global_orient=None, **kw):
        return SimpleNamespace(joints=O.smpl_forward(self.T, betas, body_pose, global_orient, pose2rot=True)[1])


def host_annotate(joints49, trans, cam_pose, cam_intrinsics, root_aa):
    j, t, P, K = joints49.numpy(), trans.numpy(), cam_pose.numpy(), cam_intrinsics.numpy()
    p = (j.astype(np.float64) + t[:, None, :]).astype(np.float32).astype(np.float64)
    q = np.einsum("nrk,njk->njr", P[:, :3, :3], p) + P[:, None, :3, 3]
    q = q / q[..., 2:3]
    uv = np.einsum("rk,njk->njr", K, q)[..., :2]
    lo, hi = uv.min(1), uv.max(1)
    Rs = torch.bmm(cam_pose[:, :3, :3].float(), O.batch_rodrigues(root_aa))
    return dict(j2d=torch.from_numpy(np.concatenate([uv, np.ones(uv.shape[:2] + (1,))], -1)), center=torch.from_numpy((hi + lo) / 2.0),
                scale=torch.from_numpy((hi - lo).max(1) / 200.0), root_aligned=O.rotmat_to_axis_angle(Rs))


def run(route, seqs, smpls, out_dir, device):
    saved = PX.annotate
    if route == "host":
        PX.annotate = host_annotate
    try:
        if device.type == "cuda":
            torch.cuda.synchronize()
        t = time.perf_counter()
        files = []
        for i, d in enumerate(seqs):
            files += PX.extract_sequence(d, i, out_dir, smpls[0], smpls[1], device)
        if device.type == "cuda":
            torch.cuda.synchronize()
        return time.perf_counter() - t, files
    finally:
        PX.annotate = saved


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--sequences", type=int, default=24)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("pw3d_extract_rate measures on the GPU: no device found")
    torch.set_num_threads(a.threads)
    dev = torch.device("cuda:0")
    tabs = [assets.make_synthetic_smpl(1), assets.make_synthetic_smpl(2)]
    legs = dict(device=([SMPL(tables=t).to(dev) for t in tabs], dev), host=([HostSMPL(t) for t in tabs], torch.device("cpu")))
    seqs = [make_sequence(i, PEOPLE[i % len(PEOPLE)]) for i in range(a.sequences)]
    tracks = sum(len(d["poses"]) for d in seqs)
    frames = int(sum(int(v.sum()) for d in seqs for v in d["campose_valid"]))
    lines = [f"3DPW extraction, synthetic set: {len(seqs)} sequences, {tracks} person-tracks, {frames} person-frames; {a.rounds} alternating "
             f"rounds after one warm-up sequence per route; host route on {a.threads} threads"]
    secs = {k: [] for k in legs}
    with tempfile.TemporaryDirectory() as tmp:
        for k, (smpls, d) in legs.items():
            run(k, seqs[:1], smpls, os.path.join(tmp, "warm_" + k), d)
        last = {}
        for r in range(a.rounds):
            for k, (smpls, d) in legs.items():
                s, last[k] = run(k, seqs, smpls, os.path.join(tmp, k), d)
                secs[k].append(s)
                print(f"round {r} {k}: {s:.3f} s", flush=True)
        worst = {}
        for fa, fb in zip(last["device"], last["host"]):
            x, y = np.load(fa), np.load(fb)
            for key in ("j3d", "j2d", "center", "scale", "pose"):
                worst[key] = max(worst.get(key, 0.0), float(np.abs(x[key].astype(np.float64) - y[key]).max()))
    res = dict(sequences=len(seqs), tracks=tracks, person_frames=frames, threads=a.threads, routes_differ=worst)
    for k, v in secs.items():
        res[k] = dict(seconds_median=float(np.median(v)), seconds_min=float(min(v)), seconds_max=float(max(v)),
                      person_frames_per_second=frames / float(np.median(v)))
        lines.append(f"{k:7s} {res[k]['seconds_median']:8.3f} s for the set (min {min(v):.3f}, max {max(v):.3f})   "
                     f"{res[k]['person_frames_per_second']:10.0f} person-frames / s")
    lines.append(f"ratio of medians (host / device): {res['host']['seconds_median'] / res['device']['seconds_median']:.2f}")
    lines.append("largest deviation between the two routes' files: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
