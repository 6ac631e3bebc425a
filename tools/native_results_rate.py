#!/usr/bin/env python3
"""What overlays (--save_res) and prediction dumps (--dump_predictions) cost with --native_results 1, on synthetic frames.  One
process, a warm-up, then --frames frame steps per leg; prints one JSON line per part.

  part 1  one sequence, default term set, --save_res 1: the autograd path (native_results 0 - what such a run did before the flag
          existed) against the native stepper with the result ring (native_results 1).  The one like-for-like comparison.
  part 2  32 sequences in lockstep, frame-loss set, native_results 1: save_res 0 / save_res 1 / dump_predictions 1.  Per leg the
          wall clock, and inside it the GPU time of the ragged overlay launches (events) and the host time spent encoding PNGs /
          writing dumps to disk (PIL's and joblib's own calls, timed on the host).
  part 3  32 meshes over 1920 x 1080 frames: ONE ragged launch (with and without the per-mesh pixel box) against 32 launches of the
          uniform entry, event-timed.  The mesh: tools/render_times.py's ellipsoid with SMPL's counts, or --soup (the synthetic
          SMPL's random-triple faces, hundreds deep at every pixel - the stress case).
  part 4  --overlay_format png against jpg (the device JPEG encoder of csrc/jpeg.hip): 1 and 32 sequences with --save_res 1 on the
          native stepper, the two legs alternating over --rounds rounds; median step time with min .. max.

usage:  timeout 900 python tools/native_results_rate.py [--part 1|2|3|4|all (= 1 - 3)] [--frames 200] [--warmup 10] [--rounds 3] [--soup]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dynaboa_amd import assets, benchmark as DB, native_step as NS      # noqa: E402
from dynaboa_amd.base_adaptor import synthetic_bundle                   # noqa: E402
from dynaboa_amd.render import Renderer                                 # noqa: E402


def make(opts, r, expdir):
    o = DB.parser.parse_args([])
    for k, v in opts.items():
        setattr(o, k, v)
    o.expdir, o.expname, o.deferred_metrics = expdir, "rate", 1
    return DB.Adaptor(o, synthetic_bundle(seed=22 + r, identity_pose=False, randomize_norm=True, smpl_seed=0), device="cuda:0")


class HostClock:
    """Accumulates the host time of PIL's Image.save and joblib.dump, and the GPU time of Renderer.render_many (events)."""

    def __init__(self):
        import joblib
        from PIL import Image
        self.png = self.dump = 0.0
        self.events = []
        self._save, self._dump, self._many = Image.Image.save, joblib.dump, Renderer.render_many
        clock = self

        def save(img, *a, **k):
            t = time.perf_counter()
            try:
                return clock._save(img, *a, **k)
            finally:
                clock.png += time.perf_counter() - t

        def dump(*a, **k):
            t = time.perf_counter()
            try:
                return clock._dump(*a, **k)
            finally:
                clock.dump += time.perf_counter() - t

        def many(r, *a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = clock._many(r, *a, **k)
            e1.record()
            clock.events.append((e0, e1))
            return out
        Image.Image.save, joblib.dump, Renderer.render_many = save, dump, many

    def reset(self):
        self.png = self.dump = 0.0
        self.events = []

    def render_ms(self):
        torch.cuda.synchronize()
        return sum(a.elapsed_time(b) for a, b in self.events)


def part1(a, clock):
    frames = [{k: v.to("cuda:0") for k, v in assets.make_frame(i, 1, seed=22).items()} for i in range(16)]
    out = dict(part=1, what="one sequence, default term set, save_res 1", frames=a.frames, warmup=a.warmup)
    for leg, nr in (("autograd_path", 0), ("native_results", 1)):
        with tempfile.TemporaryDirectory() as tmp:
            ad = make(dict(save_res=1, native_results=nr), 0, tmp)
            ad.reset_records(a.frames + a.warmup)

            def step(i):
                ad.global_step, ad.fit_losses = i, {}
                ad.model.eval()
                ad.adaptation(frames[i % 16])
            for i in range(a.warmup):
                step(i)
            torch.cuda.synchronize()
            clock.reset()
            t0 = time.perf_counter()
            for i in range(a.frames):
                step(a.warmup + i)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert (ad._native is not None) == bool(nr)
            assert len(os.listdir(os.path.join(tmp, "rate", "image"))) == a.frames + a.warmup
            out[leg] = dict(frames_per_s=round(a.frames / dt, 2), ms_per_frame=round(1e3 * dt / a.frames, 3),
                            png_ms_per_frame=round(1e3 * clock.png / a.frames, 3))
    print(json.dumps(out), flush=True)


def part2(a, clock):
    S = a.sequences
    NS.set_replica_policy(True)
    frames = [[{k: v.to("cuda:0") for k, v in assets.make_frame(100 * r + i, 1, seed=22).items()} for i in range(4)] for r in range(S)]
    base = dict(vars(DB.frame_only_options(inner_step=1)), native_results=1)
    out = dict(part=2, what=f"{S} sequences, frame-loss set, native_results 1", steps=a.frames, warmup=a.warmup)
    for leg, over in (("save_res_0", {}), ("save_res_1", dict(save_res=1)), ("dump_predictions_1", dict(dump_predictions=1))):
        with tempfile.TemporaryDirectory() as tmp:
            ads = [make(dict(base, **over), r, tmp) for r in range(S)]
            grp = NS.ReplicaGroup(ads, a.frames + a.warmup)
            step = lambda i: grp.step([frames[r][i % 4] for r in range(S)], i, result_steps=[i * S + r for r in range(S)])
            for i in range(a.warmup):
                step(i)
            torch.cuda.synchronize()
            clock.reset()
            t0 = time.perf_counter()
            for i in range(a.frames):
                step(a.warmup + i)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            grp.flush_metrics()
            n = a.frames * S
            out[leg] = dict(frames_per_s=round(n / dt, 1), ms_per_step=round(1e3 * dt / a.frames, 3),
                            overlay_gpu_ms_per_step=round(clock.render_ms() / a.frames, 3),
                            png_host_ms_per_step=round(1e3 * clock.png / a.frames, 3),
                            dump_host_ms_per_step=round(1e3 * clock.dump / a.frames, 3))
            del grp, ads
    print(json.dumps(out), flush=True)


def part3(a):
    from render_times import timed, uv_ellipsoid
    from dynaboa_amd import _lib
    from dynaboa_amd._abi import check
    from dynaboa_amd.hmr import stream_of
    from dynaboa_amd.render import RenderDesc
    import ctypes
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    if a.soup:
        t = assets.make_synthetic_smpl(0)
        v, f = t["v_template"].astype(np.float32), t["faces"]
        v = v / np.abs(v[:, :2]).max() * 0.85
    else:
        v, f = uv_ellipsoid()
    N, H, W = 32, 1080, 1920
    verts = torch.from_numpy(np.stack([v * s for s in rng.uniform(0.8, 1.0, N)]).astype(np.float32)).to(dev)
    # a person about 600 px tall somewhere in the frame: scale = 600 / (W, H), the shift keeps the box inside
    cam = torch.from_numpy(np.stack([np.full(N, 600.0 / W), np.full(N, 600.0 / H), rng.uniform(-1.5, 1.5, N), rng.uniform(-0.5, 0.5, N)], 1)
                           .astype(np.float32)).to(dev)
    frames = torch.from_numpy(rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)).to(dev)
    r = Renderer(resolution=(W, H), faces=f, device=dev)
    want = [r.render(frames[i], verts[i], cam[i]) for i in range(N)]
    lib = _lib.load()
    faces, ptr, idx = r._adjacency(int(verts.shape[1]), dev)
    outs = [torch.empty(H, W, 3, dtype=torch.uint8, device=dev) for _ in range(N)]
    desc = (RenderDesc * N)(*[RenderDesc(verts[i].data_ptr(), frames[i].data_ptr(), outs[i].data_ptr(), H, W) for i in range(N)])
    ws = torch.empty(int(lib.dyb_render_var_workspace_bytes(N, int(verts.shape[1]), int(faces.shape[0]))), dtype=torch.uint8, device=dev)

    def ragged(flags):
        check(lib.dyb_render_meshes_var(ctypes.cast(desc, ctypes.c_void_p), faces.data_ptr(), ptr.data_ptr(), idx.data_ptr(), cam.data_ptr(),
                                        1.0, 1.0, 0.9, N, int(verts.shape[1]), int(faces.shape[0]), flags, ws.data_ptr(), ws.numel(),
                                        stream_of(cam)), "dyb_render_meshes_var")
    out = dict(part=3, what=f"{N} meshes ({'soup' if a.soup else 'ellipsoid'}, {len(f)} faces) over {W}x{H}", reps=a.reps)
    for flags in (0, 1):
        ragged(flags)
        torch.cuda.synchronize()
        assert all(torch.equal(o, w) for o, w in zip(outs, want))
    covered = float(np.mean([float((w != fr).any(-1).float().mean()) for w, fr in zip(want, frames)]))
    out["covered_fraction"] = round(covered, 4)
    wsu = torch.empty(int(lib.dyb_render_workspace_bytes(1, int(verts.shape[1]), int(faces.shape[0]))), dtype=torch.uint8, device=dev)

    def uniform():                                   # one call of the uniform entry per mesh, image output only, nothing allocated
        for i in range(N):
            check(lib.dyb_render_meshes(verts[i].data_ptr(), faces.data_ptr(), ptr.data_ptr(), idx.data_ptr(), cam[i].data_ptr(),
                                        frames[i].data_ptr(), 1.0, 1.0, 0.9, outs[i].data_ptr(), None, None, 1, int(verts.shape[1]),
                                        int(faces.shape[0]), H, W, wsu.data_ptr(), wsu.numel(), stream_of(cam)), "dyb_render_meshes")
    for name, fn in (("uniform_32_launches", uniform),
                     ("ragged_no_box", lambda: ragged(1)), ("ragged_box", lambda: ragged(0))):
        p50, lo = timed(fn, a.reps)
        out[name] = dict(ms_median=round(p50, 3), ms_min=round(lo, 3))
    print(json.dumps(out), flush=True)


def part4(a, clock):
    """--overlay_format png against jpg, end to end: S sequences in lockstep (S = 1 and --sequences), frame-loss set, native_results 1,
    save_res 1 over the 224 x 224 crops.  Both groups live side by side and take turns: --rounds rounds of --frames steps each,
    alternating; the median step time with its spread (min .. max) per leg."""
    import statistics
    NS.set_replica_policy(True)
    base = dict(vars(DB.frame_only_options(inner_step=1)), native_results=1, save_res=1)
    for S in sorted({1, a.sequences}):
        frames = [[{k: v.to("cuda:0") for k, v in assets.make_frame(100 * r + i, 1, seed=22).items()} for i in range(4)] for r in range(S)]
        out = dict(part=4, what=f"{S} sequences, frame-loss set, native_results 1, save_res 1: overlay_format png / jpg",
                   steps=a.frames, warmup=a.warmup, rounds=a.rounds)
        with tempfile.TemporaryDirectory() as tmp:
            legs, at = {}, {}
            for leg in ("png", "jpg"):
                ads = [make(dict(base, overlay_format=leg), r, os.path.join(tmp, leg)) for r in range(S)]
                legs[leg] = NS.ReplicaGroup(ads, a.rounds * a.frames + a.warmup) if S > 1 else ads[0]
                if S == 1:
                    ads[0].reset_records(a.rounds * a.frames + a.warmup)
                at[leg] = 0

            def step(leg):
                i = at[leg]
                at[leg] += 1
                if S > 1:
                    legs[leg].step([frames[r][i % 4] for r in range(S)], i, result_steps=[i * S + r for r in range(S)])
                else:
                    ad = legs[leg]
                    ad.global_step, ad.fit_losses = i, {}
                    ad.model.eval()
                    ad.adaptation(frames[0][i % 4])
            for leg in legs:
                for _ in range(a.warmup):
                    step(leg)
            torch.cuda.synchronize()
            times = {leg: [] for leg in legs}
            for _ in range(a.rounds):
                for leg in legs:
                    t0 = time.perf_counter()
                    for _ in range(a.frames):
                        step(leg)
                    torch.cuda.synchronize()
                    times[leg].append(1e3 * (time.perf_counter() - t0) / a.frames)
            for leg in legs:
                n = len(os.listdir(os.path.join(tmp, leg, "rate", "image")))
                assert n == S * (a.rounds * a.frames + a.warmup), (leg, n)
                out[leg] = dict(ms_per_step_median=round(statistics.median(times[leg]), 3), ms_min=round(min(times[leg]), 3),
                                ms_max=round(max(times[leg]), 3))
            del legs
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["1", "2", "3", "4", "all"], help="all = parts 1 - 3; part 4 only when named")
    ap.add_argument("--rounds", type=int, default=3, help="part 4: alternating rounds per leg")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sequences", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--soup", action="store_true")
    a = ap.parse_args()
    clock = HostClock()
    if a.part in ("1", "all"):
        part1(a, clock)
    if a.part in ("2", "all"):
        part2(a, clock)
    if a.part in ("3", "all"):
        part3(a)
    if a.part == "4":                                # not part of "all": that stays what it was
        part4(a, clock)


if __name__ == "__main__":
    main()
