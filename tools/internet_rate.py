#!/usr/bin/env python3
"""What the batched crop (``datasets.preprocess_frames`` / ``dyb_crop_resize_normalize_many``) is worth, on 1280 x 720 frames.  One
process; prints one JSON line per measurement.

  part 1  n = 1, 8, 32 crops from resident frames (person boxes of 260 .. 650 px, a few hanging over the edge, two people per frame):
          ``preprocess_frames`` against a loop of the unchanged ``preprocess_frame``.  Per leg the time of one round - host clock
          around `reps` rounds ending in a device synchronise - and the launch / call counts (by construction: the single entry is
          one C call with three launches per crop; the many entry one C call with three launches and one host-to-device copy of
          the descriptors per 64 crops).
  part 2  the internet driver's lockstep step at S = 1, 8, 32 tracks of one synthetic video (default term set on the native stepper,
          no result files): frames per second of ``ReplicaGroup.step`` fed by ``internet.TrackGroupLoader`` with the batched crop
          and with one ``preprocess_frame`` per crop, the legs alternating.  S = 1 is one sequence through ``Adaptor.excute``
          (its loader crops singly either way: the base line).

usage:  timeout 900 python tools/internet_rate.py [--part 1|2|all] [--reps 200] [--frames 24] [--tracks 1,8,32]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dynaboa_amd import datasets as D, internet as I, native_step as NS      # noqa: E402
from dynaboa_amd.base_adaptor import synthetic_bundle                        # noqa: E402

DEV = "cuda:0"
H, W = 720, 1280
# a standing person in units of its height, COCO-17 order (tools/make_golden_internet.py's)
POSE = np.array([[0.00, 0.06], [0.02, 0.04], [-0.02, 0.04], [0.05, 0.05], [-0.05, 0.05], [0.11, 0.18], [-0.11, 0.18], [0.15, 0.34],
                 [-0.15, 0.34], [0.17, 0.48], [-0.17, 0.48], [0.07, 0.52], [-0.07, 0.52], [0.08, 0.75], [-0.08, 0.75], [0.09, 0.97],
                 [-0.09, 0.97]])


def frame(seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([(xx // 3 + seed) % 256, (yy // 2 + 3 * seed) % 256, ((xx + yy) // 5) % 256], -1).astype(np.int32)
    return (img + rng.integers(-20, 20, img.shape)).clip(0, 255).astype(np.uint8)


def part1(reps):
    rng = np.random.default_rng(1)
    for n in (1, 8, 32):
        frames = [torch.from_numpy(frame(i)).to(DEV) for i in range((n + 1) // 2)]
        which = [i // 2 for i in range(n)]
        centers = [np.array([rng.uniform(100, W - 100), rng.uniform(200, H - 200)]) for _ in range(n)]
        scales = [float(rng.uniform(1.3, 3.25)) for _ in range(n)]
        out = torch.empty(n, 3, 224, 224, device=DEV)

        def many():
            D.preprocess_frames([frames[w] for w in which], centers, scales, out=out)

        def loop():
            for i in range(n):
                D.preprocess_frame(frames[which[i]], centers[i], scales[i], out=out[i])
        many()
        a = out.clone()
        loop()
        assert torch.equal(a, out)
        t = {"many": [], "loop": []}
        for _ in range(3):                           # alternate the legs
            for name, fn in (("many", many), ("loop", loop)):
                for _ in range(10):
                    fn()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize()
                t[name].append((time.perf_counter() - t0) / reps * 1e3)
        print(json.dumps(dict(part=1, n=n, frame=[H, W], reps=reps, ms_many=round(min(t["many"]), 4), ms_loop=round(min(t["loop"]), 4),
                              ms_many_all=[round(x, 4) for x in t["many"]], ms_loop_all=[round(x, 4) for x in t["loop"]],
                              launches_many=3, copies_many=1, c_calls_many=1, launches_loop=3 * n, c_calls_loop=n)), flush=True)


def make_video(root, tracks, nframes):
    """<root>/vid.json + images/vid/*.png: `tracks` people walking through `nframes` frames; every detection passes --extract."""
    from PIL import Image
    rng = np.random.default_rng(5)
    os.makedirs(os.path.join(root, "images", "vid"))
    x0, h0 = rng.uniform(80, W - 80, tracks), rng.uniform(300, 560, tracks)
    dets = []
    for f in range(nframes):
        Image.fromarray(frame(100 + f)).save(os.path.join(root, "images", "vid", f"{f:06d}.png"))
        for tr in range(tracks):
            kp = np.concatenate([np.array([x0[tr] + 4 * f, 80.0]) + POSE * h0[tr] + rng.normal(0, 1.5, (17, 2)), rng.uniform(0.5, 0.95, (17, 1))], 1)
            dets.append(dict(image_id=f"{f:06d}.png", keypoints=[float(v) for v in kp.ravel()], score=3.0, idx=[float(tr)]))
    with open(os.path.join(root, "vid.json"), "w") as fh:
        json.dump(dets, fh)
    I.internet_data_extract(root)


def part2(tracks_list, nframes):
    import copy
    bundle = synthetic_bundle(seed=22, identity_pose=False, randomize_norm=True, smpl_seed=0)
    NS.set_replica_policy(True)
    for S in tracks_list:
        with tempfile.TemporaryDirectory() as root:
            make_video(root, S, nframes)
            o = I.parser.parse_args(["--internet_root", root, "--expdir", root, "--expname", "rate", "--split_tracks", "1",
                                     "--dump_predictions", "0"])
            ds = I.InternetDataset(o, device=DEV)
            assert len(ds.sequences) == S and all(s["frames"] == nframes for s in ds.sequences)
            res = dict(part=2, tracks=S, frames_per_track=nframes)
            for leg in (("batched", "single", "batched", "single") if S > 1 else ("single", "single")):
                ads = [I.Adaptor(copy.copy(o), bundle, DEV) for _ in range(S)]
                warm = 4
                if S == 1:
                    ad = ads[0]
                    it = iter(D.FrameLoader(ds, batch_size=1, workers=4, indices=ds.sequences[0]["rows"]))
                    ad.reset_records(nframes)
                    for step in range(nframes):
                        if step == warm:
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                        b = next(it)
                        ad.global_step = step
                        ad.fit_losses = {}
                        ad.adaptation(b)
                else:
                    grp = NS.ReplicaGroup(ads, nframes)
                    for step, items in enumerate(I.TrackGroupLoader(ds, ds.sequences, workers=4, batched=leg == "batched")):
                        if step == warm:
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                        batches = [None] * S
                        for si, b in items:
                            batches[si] = b
                        grp.step(batches, step)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / (nframes - warm)
                res.setdefault(f"ms_step_{leg}", []).append(round(dt * 1e3, 3))
                del ads
            for leg in ("batched", "single"):
                if f"ms_step_{leg}" in res:
                    res[f"frames_per_s_{leg}"] = round(S / (min(res[f"ms_step_{leg}"]) * 1e-3), 1)
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--tracks", default="1,8,32")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("internet_rate.py measures on the GPU; there is none")
    if a.part in ("1", "all"):
        part1(a.reps)
    if a.part in ("2", "all"):
        part2([int(x) for x in a.tracks.split(",")], a.frames)
