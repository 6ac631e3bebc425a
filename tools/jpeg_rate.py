#!/usr/bin/env python3
"""What a finished overlay costs on its way to a file, per picture, for 1, 8 and 32 pictures at 1280 x 720 and 1920 x 1080 - over
rendered overlays (a mesh drawn by the rasteriser over a synthetic photograph-like frame: smooth shading, blur-scale texture and
sensor noise of sigma 2 in EVERY pixel; not white noise, which no encoder meets in practice), in one process.  The noise decides the
PNG leg: deflate cannot shorten it and still searches, so PNG costs 25 x what round 11 saw on a flat frame (5 - 6 ms at 1280 x 720);
a camera frame lies between the two and none was measured - quote the PNG column with that beside it.

  a png      today's path: .cpu() and PIL's PNG save, one host thread
  b pil_jpg  .cpu() and PIL's JPEG save at the same quality and subsampling
  c device   JpegEncoder.save: dyb_jpeg_encode_many, one wait for the lengths, the used bytes to the host, the files written

Host clock around each leg (every leg ends in files on disk, c after its device waits); the legs alternate inside each of --rounds
rounds after a warm-up, medians with min .. max.  For c also: the time of the six launches alone (events around
dyb_jpeg_encode_many itself: no copy, no wait inside the bracket), the bytes the design moves per picture - counted from the shapes: the pixels once, 134 bytes per
block written by the transform (coefficients, DC, bit count) and read again by the emit, 10 bytes per block through the bits
kernel, the unstuffed stream written, read and written again stuffed - against the HBM rate, and the bytes copied to the host.
Writes profiles/r21_jpeg_rate.txt when --out is given.  Records, not thresholds.

usage:  timeout 600 python tools/jpeg_rate.py [--rounds 3] [--warm 1] [--quality 90] [--subsampling 444] [--out profiles/r21_jpeg_rate.txt]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dynaboa_amd.jpeg import JpegEncoder          # noqa: E402
from dynaboa_amd.render import Renderer           # noqa: E402

DEV = "cuda:0"
HBM_BYTES_PER_S = 6.3e12                           # what a streaming kernel reaches on this part (8.0e12 on paper)


def photo(H, W, seed):
    """A frame with a photograph's statistics, roughly: large smooth structures, texture at a few pixels' scale, mild noise."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = torch.zeros(1, 3, H, W, device=DEV)
    for scale, amp in ((64, 70.0), (16, 35.0), (4, 14.0)):
        coarse = torch.randn(1, 3, H // scale + 2, W // scale + 2, device=DEV, generator=g)
        out += amp * torch.nn.functional.interpolate(coarse, size=(H, W), mode="bicubic", align_corners=False)
    out += 128.0 + 2.0 * torch.randn(1, 3, H, W, device=DEV, generator=g)
    return out.clamp(0, 255).to(torch.uint8)[0].permute(1, 2, 0).contiguous()


def overlays(n, H, W):
    from render_times import uv_ellipsoid
    v, f = uv_ellipsoid()
    rng = np.random.default_rng(n + H)
    verts = [torch.from_numpy((v * s).astype(np.float32)).to(DEV) for s in rng.uniform(0.8, 1.0, n)]
    cam = torch.from_numpy(np.stack([np.full(n, 600.0 / W), np.full(n, 600.0 / H), rng.uniform(-1.0, 1.0, n), rng.uniform(-0.3, 0.3, n)], 1)
                           .astype(np.float32)).to(DEV)
    frames = [photo(H, W, 7 * i + H) for i in range(n)]
    r = Renderer(resolution=(W, H), faces=f, device=DEV)
    pics = []
    for lo in range(0, n, 64):
        pics += r.render_many(frames[lo:lo + 64], verts[lo:lo + 64], cam[lo:lo + 64], color=(205 / 255.0, 129 / 255.0, 98 / 255.0))
    return pics


def main():
    from PIL import Image
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--warm", type=int, default=1)
    p.add_argument("--quality", type=int, default=90)
    p.add_argument("--subsampling", type=int, default=444, choices=[444, 420])
    p.add_argument("--out", type=str, default=None)
    o = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_rate: needs the GPU (no fall-back: a CPU time says nothing about the device)")
    enc = JpegEncoder(DEV, o.quality, o.subsampling)
    pil_sub = 0 if o.subsampling == 444 else 2
    lines = [f"# {torch.cuda.get_device_name(0)}; rendered overlays, quality {o.quality}, {o.subsampling}; ms per picture, median of "
             f"{o.rounds} alternating rounds after {o.warm} warm-up (min .. max); host clock, files written; synthetic frames with "
             "sigma-2 noise in every pixel (PNG's worst case short of white noise; no camera frame measured)"]
    records = []
    with tempfile.TemporaryDirectory() as tmp:
        for (W, H) in ((1280, 720), (1920, 1080)):
            for n in (1, 8, 32):
                pics = overlays(n, H, W)
                torch.cuda.synchronize()
                names = [os.path.join(tmp, f"p{i}") for i in range(n)]

                def png():
                    for pic, name in zip(pics, names):
                        Image.fromarray(pic.cpu().numpy()).save(name + ".png")

                def pil_jpg():
                    for pic, name in zip(pics, names):
                        Image.fromarray(pic.cpu().numpy()).save(name + "_pil.jpg", quality=o.quality, subsampling=pil_sub)

                def device():
                    enc.save(pics, [name + ".jpg" for name in names])
                legs = dict(png=png, pil_jpg=pil_jpg, device=device)
                for _ in range(o.warm):
                    for fn in legs.values():
                        fn()
                times = {k: [] for k in legs}
                for _ in range(o.rounds):
                    for k, fn in legs.items():
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        times[k].append(1e3 * (time.perf_counter() - t0) / n)
                # the device leg equals libjpeg's bytes on this content too
                for name in names[:2]:
                    a, b = open(name + ".jpg", "rb").read(), open(name + "_pil.jpg", "rb").read()
                    assert a[a.rindex(b"\xff\xda"):] == b[b.rindex(b"\xff\xda"):], "device scan differs from PIL's"
                # the six launches alone: events around dyb_jpeg_encode_many itself - no copy of the lengths, no wait inside the
                # bracket (the host's time to issue the launches is, where the device is faster than that)
                caps = [H * W * 3 // 2 + 4096] * n
                ev = []
                for _ in range(o.rounds + o.warm):
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    enc._launch(pics[:64], caps[:64])
                    e1.record()
                    e1.synchronize()
                    ev.append(e0.elapsed_time(e1) / min(n, 64))
                ev = ev[o.warm:]
                enc.encode(pics)
                to_host = enc.bytes_to_host / n
                scan = to_host - 8
                nblk = 3 * ((H + 7) // 8) * ((W + 7) // 8) if o.subsampling == 444 else 6 * ((H + 15) // 16) * ((W + 15) // 16)
                moved = H * W * 3 + nblk * (134 + 10 + 134) + 3 * scan
                med = {k: statistics.median(v) for k, v in times.items()}
                dev_ms = statistics.median(ev)
                lines.append(f"{W}x{H} n={n:2d}  png {med['png']:7.3f} ({min(times['png']):.3f} .. {max(times['png']):.3f})  "
                             f"pil_jpg {med['pil_jpg']:7.3f} ({min(times['pil_jpg']):.3f} .. {max(times['pil_jpg']):.3f})  "
                             f"device {med['device']:7.3f} ({min(times['device']):.3f} .. {max(times['device']):.3f})  "
                             f"| six launches alone {dev_ms:.3f} ({min(ev):.3f} .. {max(ev):.3f}) ms/picture by events; design moves "
                             f"{moved / 1e6:.1f} MB/picture = {1e3 * moved / HBM_BYTES_PER_S:.4f} ms at 6.3 TB/s; "
                             f"{to_host / 1e3:.0f} KB/picture to the host (raw: {H * W * 3 / 1e3:.0f} KB)")
                records.append(dict(W=W, H=H, n=n, **{k: dict(median=round(med[k], 4), min=round(min(v), 4), max=round(max(v), 4))
                                                      for k, v in times.items()},
                                    encode_call_ms=round(dev_ms, 4), moved_bytes=int(moved), host_bytes=int(to_host)))
                print(lines[-1], flush=True)
                del pics
    print(json.dumps(dict(quality=o.quality, subsampling=o.subsampling, rounds=o.rounds, records=records)))
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
