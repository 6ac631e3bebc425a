#!/usr/bin/env python3
"""Cost of the device tracker (dynaboa_amd/track.py, csrc/track.hip) on V seeded videos of about 9 000 frames with 5 - 10 people of 17
joints each, in one process:

  call      dynaboa_amd.track.track_videos over all V videos: packing, ONE upload, ONE dyb_track_videos launch, one download (host clock)
  kernel    the dyb_track_videos launch alone on buffers that are already on the device (device events)
  host      a per-frame NumPy tracker of the same rule (fp32, vectorised over the frame's pairs and joints) on the first --host_videos
            videos, reported per video - a video's host time does not depend on how many others there are

One video is a dependent chain of frames on one workgroup: the device's parallelism is across videos, so the kernel leg should stay
flat from V = 1 to V = 37 while the host's grows with V.  Ids of the two routes are compared.  These are records, not thresholds.

usage:  timeout 300 python tools/track_rate.py --videos 8 [--frames 9000] [--rounds 3] [--host_videos 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dynaboa_amd import track as T            # noqa: E402

DEV = "cuda:0"
K = 17


def make_video(seed, frames):
    """5 - 10 people on random walks (about 2 pixels per frame) over a 1920 x 1080 field, each missing now and then for 1 - 30
    frames; 10 % of the joints hidden.  -> a list of (n_f, K, 3) float32 arrays."""
    rng = np.random.default_rng(seed)
    P = int(rng.integers(5, 11))
    tpl = np.stack([rng.uniform(-40, 40, (P, K)), rng.uniform(-100, 100, (P, K))], -1)
    pos = rng.uniform((200, 200), (1700, 900), (P, 2))[None] + np.cumsum(rng.normal(0, 1.5, (frames, P, 2)), 0)
    xy = tpl[None] + pos[:, :, None, :] + rng.normal(0, 0.5, (frames, P, K, 2))
    conf = np.where(rng.random((frames, P, K)) < 0.1, 0.1, rng.uniform(0.5, 0.95, (frames, P, K)))
    dense = np.concatenate([xy, conf[..., None]], -1).astype(np.float32)
    present = np.ones((frames, P), bool)
    for p in range(P):
        for start in rng.integers(0, frames, max(1, frames // 600)):
            present[start:start + int(rng.integers(1, 31)), p] = False
    return [dense[f][present[f]] for f in range(frames)]


def host_tracker(video, c_min=T.C_MIN, kappa=T.KAPPA, s_min=T.S_MIN, max_age=T.MAX_AGE, min_common=T.MIN_COMMON):
    """The rule of dyb_track_videos per frame in NumPy, float32 -> per frame the ids."""
    f32 = np.float32
    ids, last, xy, mask, area = [], [], [], [], []                     # the live tracks, in id order
    next_id, out = 0, []
    for fid, det in enumerate(video):
        keep = [i for i, l in enumerate(last) if fid - l <= max_age]
        ids, last, xy, mask, area = ([a[i] for i in keep] for a in (ids, last, xy, mask, area))
        det = det[:T.MAX_PEOPLE]
        m = det.shape[0]
        dm = det[:, :, 2] > f32(c_min)
        ok = dm.sum(1) >= min_common
        big, small = np.where(dm[..., None], det[:, :, :2], -np.inf).max(1), np.where(dm[..., None], det[:, :, :2], np.inf).min(1)
        with np.errstate(invalid="ignore"):
            da = np.where(dm.any(1), (big[:, 0] - small[:, 0]) * (big[:, 1] - small[:, 1]), 0).astype(f32)
        tr = -np.ones(m, np.int32)
        matched = np.zeros(m, bool)
        if ids and m:
            txy, tm, ta = np.stack(xy), np.stack(mask), np.array(area, f32)
            common = tm[:, None, :] & (dm & ok[:, None])[None]
            nc = common.sum(-1)
            A = np.maximum((ta[:, None] + da[None]) * f32(0.5), f32(1))
            d2 = ((txy[:, None] - det[None, :, :, :2]) ** 2).sum(-1)
            e = np.where(common, np.exp(-d2 / (f32(2) * f32(kappa) * f32(kappa) * A)[..., None]), f32(0))
            S = np.where(nc >= min_common, e.sum(-1) / np.maximum(nc, 1), 0).astype(f32)
            S[S < f32(s_min)] = -1
            while True:
                flat = int(np.argmax(S))                                # the first maximum: lower id, then lower index
                t, d = divmod(flat, m)
                if S[t, d] < 0:
                    break
                tr[d], matched[d] = ids[t], True
                xy[t], mask[t], area[t], last[t] = det[d, :, :2], dm[d], da[d], fid
                S[t, :], S[:, d] = -1, -1
        for d in range(m):
            if ok[d] and not matched[d] and len(ids) < T.MAX_PEOPLE:
                tr[d] = next_id
                ids.append(next_id); last.append(fid); xy.append(det[d, :, :2]); mask.append(dm[d]); area.append(da[d])
                next_id += 1
        out.append(tr)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--videos", type=int, default=8)
    p.add_argument("--frames", type=int, default=9000)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--host_videos", type=int, default=2)
    o = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("track_rate: needs the GPU (no fall-back: a CPU time says nothing about the device)")
    from dynaboa_amd import _lib
    from dynaboa_amd.hmr import stream_of
    V = o.videos
    videos = [make_video(100 + v, o.frames + 37 * v) for v in range(V)]
    n = sum(f.shape[0] for v in videos for f in v)
    T.track_videos(videos[:1], device=DEV)                              # warm-up: library load, first launch
    call = []
    for _ in range(o.rounds):
        t0 = time.perf_counter()
        tracks, _, counts = T.track_videos(videos, device=DEV)
        call.append((time.perf_counter() - t0) * 1e3)
    frames = [f for v in videos for f in v]
    kp = torch.from_numpy(np.concatenate(frames)).to(DEV)
    det = torch.from_numpy(np.concatenate([[0], np.cumsum([f.shape[0] for f in frames])]).astype(np.int32)).to(DEV)
    fr = torch.from_numpy(np.concatenate([[0], np.cumsum([len(v) for v in videos])]).astype(np.int32)).to(DEV)
    tr_out, vid_out = torch.empty(n, dtype=torch.int32, device=DEV), torch.empty(V, 4, dtype=torch.int32, device=DEV)
    lib, kern = _lib.load(), []
    for i in range(o.rounds + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = lib.dyb_track_videos(kp.data_ptr(), det.data_ptr(), fr.data_ptr(), None, K, T.C_MIN, T.KAPPA, T.S_MIN, T.MAX_AGE, T.MIN_COMMON,
                                  tr_out.data_ptr(), None, vid_out.data_ptr(), n, len(frames), V, stream_of(kp))
        b.record()
        b.synchronize()
        assert rc == 0
        if i:
            kern.append(a.elapsed_time(b))
    assert np.array_equal(tr_out.cpu().numpy(), np.concatenate([t for v in tracks for t in v]))
    host, differ = [], 0
    for v in range(min(V, o.host_videos)):
        t0 = time.perf_counter()
        ref = host_tracker(videos[v])
        host.append((time.perf_counter() - t0) * 1e3)
        differ += int(sum((a != b).sum() for a, b in zip(ref, tracks[v])))
    med = lambda x: statistics.median(x)
    print(f"# {torch.cuda.get_device_name(0)}; V = {V} videos of {len(videos[0])} .. {len(videos[-1])} frames, {n} detections of {K} joints, "
          f"{sum(c['started'] for c in counts)} tracks started; ms, median of {o.rounds} rounds (min .. max)")
    print(f"call    {med(call):10.2f} ({min(call):.2f} .. {max(call):.2f})   track_videos: pack + upload + launch + download, all V videos")
    print(f"kernel  {med(kern):10.2f} ({min(kern):.2f} .. {max(kern):.2f})   the dyb_track_videos launch alone, all V videos")
    print(f"host    {med(host):10.2f} ({min(host):.2f} .. {max(host):.2f})   NumPy, PER VIDEO ({len(host)} measured); x V = {med(host) * V:.0f} ms")
    print(f"host x V / call = {med(host) * V / med(call):.2f}; host x V / kernel = {med(host) * V / med(kern):.2f}; "
          f"ids that differ between the routes on the measured videos: {differ}")
    print(json.dumps(dict(videos=V, frames=o.frames, detections=n, rounds=o.rounds, call_ms=round(med(call), 3), kernel_ms=round(med(kern), 3),
                          host_ms_per_video=round(med(host), 3), host_videos=len(host), ids_differ=differ)))


if __name__ == "__main__":
    main()
