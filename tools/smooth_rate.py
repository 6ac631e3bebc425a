#!/usr/bin/env python3
"""Cost of the temporal smoothers (dynaboa_amd/smooth.py, csrc/smooth.hip) at the size of a whole 3DPW test run - 35 000 frames of 24
joint rotations, 10 betas and a 3-channel camera in 37 ragged sequences, half window 4 - on synthetic rotations, in one process:

  kernel    dynaboa_amd.smooth.smooth_sequences: ONE dyb_smooth_sequences call, the upload of the 38 offsets included
  torch     a plain torch composition of the same filter: the four-branch quaternion formula with torch.where, then per tap a shifted
            view masked by the sequence ids, the hemisphere flip, the weighted sum, the normalisation and the matrix formula; the
            betas and camera as masked weighted means (2 h + 1 passes over [n][24][4] intermediates)
  one_euro  one dyb_one_euro_step through OneEuro.step at R = 1 and at R = 32 sequences

Device events around each leg, every leg warmed up, the legs alternating inside each of --rounds rounds, medians reported with the
spread (min .. max); kernel and torch results are compared.  These are records, not thresholds.

usage:  timeout 300 python tools/smooth_rate.py [--frames 35000] [--sequences 37] [--half_window 4] [--rounds 9] [--warm 3]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dynaboa_amd import smooth as S           # noqa: E402

DEV = "cuda:0"


def ragged_lengths(n, s, seed=19):
    """s lengths between roughly a third and three times the mean, summing to n."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.3, 3.0, s)
    ln = np.maximum(3, np.floor(w / w.sum() * n)).astype(np.int64)
    ln[-1] += n - ln.sum()
    assert ln.min() >= 3 and ln.sum() == n
    return ln.tolist()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def rodrigues(aa):
    th = aa.norm(dim=-1, keepdim=True).clamp(min=1e-12)
    k = aa / th
    x, y, z = k.unbind(-1)
    c, s = torch.cos(th[..., 0]), torch.sin(th[..., 0])
    C = 1 - c
    return torch.stack([c + x * x * C, x * y * C - z * s, x * z * C + y * s, y * x * C + z * s, c + y * y * C, y * z * C - x * s,
                        z * x * C - y * s, z * y * C + x * s, c + z * z * C], -1)


def rot_to_quat(R):
    r00, r01, r02, r10, r11, r12, r20, r21, r22 = R.unbind(-1)
    d2, d01, d0n1 = r22 < 1e-6, r00 > r11, r00 < -r11
    b0, b1, b2 = d2 & d01, d2 & ~d01, ~d2 & d0n1
    t0, t1, t2, t3 = 1 + r00 - r11 - r22, 1 - r00 + r11 - r22, 1 - r00 - r11 + r22, 1 + r00 + r11 + r22
    u0 = torch.stack([r21 - r12, t0, r10 + r01, r02 + r20], -1)
    u1 = torch.stack([r02 - r20, r10 + r01, t1, r21 + r12], -1)
    u2 = torch.stack([r10 - r01, r02 + r20, r21 + r12, t2], -1)
    u3 = torch.stack([t3, r21 - r12, r02 - r20, r10 - r01], -1)
    u = torch.where(b0[..., None], u0, torch.where(b1[..., None], u1, torch.where(b2[..., None], u2, u3)))
    t = torch.where(b0, t0, torch.where(b1, t1, torch.where(b2, t2, t3)))
    return u * (0.5 / t.sqrt())[..., None]


def quat_to_rot(q):
    w, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                        2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=35000)
    p.add_argument("--sequences", type=int, default=37)
    p.add_argument("--half_window", type=int, default=4)
    p.add_argument("--rounds", type=int, default=9)
    p.add_argument("--warm", type=int, default=3)
    o = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("smooth_rate: needs the GPU (no fall-back: a CPU time says nothing about the device)")
    n, nseq, h, J = o.frames, o.sequences, o.half_window, 24
    lengths = ragged_lengths(n, nseq)
    g = torch.Generator(device=DEV).manual_seed(19)
    t = torch.arange(n, device=DEV, dtype=torch.float32)[:, None, None]
    aa = 0.6 * torch.sin(0.06 * t + 6 * torch.rand(1, J, 3, device=DEV, generator=g)) + 0.05 * torch.randn(n, J, 3, device=DEV, generator=g)
    rot = rodrigues(aa).contiguous()
    betas = torch.randn(n, 10, device=DEV, generator=g)
    cam = torch.randn(n, 3, device=DEV, generator=g)
    seq_id = torch.repeat_interleave(torch.arange(nseq, device=DEV), torch.tensor(lengths, device=DEV))
    w = torch.from_numpy(S.gaussian_weights(h)).to(DEV)

    def kernel():
        return S.smooth_sequences(rot, betas, cam, lengths=lengths, half_window=h)

    def composed():
        q = rot_to_quat(rot)
        s = torch.zeros_like(q)
        sb, sc, ws = torch.zeros_like(betas), torch.zeros_like(cam), torch.zeros(n, device=DEV)
        for k in range(-h, h + 1):
            lo, hi = max(0, -k), min(n, n - k)                   # centres lo .. hi - 1 read tap centre + k
            ok = (seq_id[lo:hi] == seq_id[lo + k:hi + k]).float() * w[k + h]
            qk = q[lo + k:hi + k]
            sign = torch.where((qk * q[lo:hi]).sum(-1) < 0, -1.0, 1.0)
            s[lo:hi] += (ok[:, None] * sign)[..., None] * qk
            sb[lo:hi] += ok[:, None] * betas[lo + k:hi + k]
            sc[lo:hi] += ok[:, None] * cam[lo + k:hi + k]
            ws[lo:hi] += ok
        return quat_to_rot(s / s.norm(dim=-1, keepdim=True)), sb / ws[:, None], sc / ws[:, None]

    filters = {R: S.OneEuro(R, beta=0.3, device=DEV) for R in (1, 32)}

    def euro(R):
        return lambda: filters[R].step(rot[:R], betas[:R], cam[:R])

    legs = dict(kernel=kernel, torch=composed, one_euro_1=euro(1), one_euro_32=euro(32))
    for _ in range(o.warm):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(o.rounds):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            times[name].append(timed(fn)[0])
    a, b = kernel(), composed()
    torch.cuda.synchronize()
    diff = [float((x - y).abs().max()) for x, y in zip(a, b)]
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f"# {torch.cuda.get_device_name(0)}; {n} frames x {J} joints + 10 betas + 3 camera channels in {nseq} sequences of "
          f"{min(lengths)} .. {max(lengths)} frames, half window {h}; ms, median of {o.rounds} alternating rounds after {o.warm} warm-up "
          "calls (min .. max)")
    for k, v in times.items():
        print(f"{k:12s} {med[k]:8.3f} ({min(v):.3f} .. {max(v):.3f})")
    print(f"torch / kernel = {med['torch'] / med['kernel']:.2f}; max |kernel - torch| rotmat {diff[0]:.1e}, betas {diff[1]:.1e}, cam {diff[2]:.1e}")
    print(json.dumps(dict(frames=n, sequences=nseq, joints=J, half_window=h, rounds=o.rounds, warm=o.warm,
                          **{k: dict(median_ms=round(med[k], 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4)) for k, v in times.items()},
                          max_abs_diff=diff)))


if __name__ == "__main__":
    main()
