#!/usr/bin/env python3
"""Time of the sequence-metric part of the metric flush (dynaboa_amd/benchmark.py: flush_metrics_of with --seq_metrics 1) at the size of
a whole 3DPW test run: 35 000 frames of 14 joints in 37 ragged sequences, on synthetic joints.  Two ways to the same numbers - per
frame MPJPE, PA-MPJPE, PCK@150mm, AUC, acceleration error and its counted flag, per sequence their means -, measured in one process:

  kernel  dynaboa_amd.pose_utils.sequence_metrics_device: ONE dyb_seq_metrics call (csrc/seq_metrics.hip: a launch over the frames, a
          reduction per sequence), as the flush issues it - the uploads of the 38 offsets and 31 thresholds included
  torch   what the commit before this feature could do on the device: dyb_pa_mpjpe for the Procrustes error plus the torch
          composition of the rest (norms, comparisons against the thresholds - an [n][J][31] intermediate -, second differences
          masked at the sequence boundaries, per-sequence sums by index_add_: floating-point atomics, not deterministic)

Device events around each leg, every leg warmed up, the legs alternating inside each of --rounds rounds, medians reported with the
spread (min .. max).  The two results are compared (largest absolute difference per column).  Nothing else of the flush is timed:
the adaptation loop is untouched by the feature and the flush runs once per run.

usage:  timeout 300 python tools/seq_metrics_rate.py [--frames 35000] [--sequences 37] [--rounds 9] [--warm 3]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dynaboa_amd import pose_utils as PU      # noqa: E402

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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=35000)
    p.add_argument("--sequences", type=int, default=37)
    p.add_argument("--rounds", type=int, default=9)
    p.add_argument("--warm", type=int, default=3)
    o = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seq_metrics_rate: needs the GPU (no fall-back: a CPU time says nothing about the device)")
    n, S, J = o.frames, o.sequences, 14
    lengths = ragged_lengths(n, S)
    g = torch.Generator(device=DEV).manual_seed(19)
    gt = torch.randn(n, J, 3, device=DEV, generator=g) * 0.3
    pred = gt + torch.randn(n, J, 3, device=DEV, generator=g) * 0.04
    seq_id = torch.repeat_interleave(torch.arange(S, device=DEV), torch.tensor(lengths, device=DEV))
    thr = torch.tensor(PU.AUC_THRESHOLDS, dtype=torch.float32, device=DEV)
    count = torch.tensor(lengths, dtype=torch.float32, device=DEV)

    def kernel():
        return PU.sequence_metrics_device(pred, gt, lengths)

    def composed():
        d = (pred - gt).norm(dim=-1)
        cols = torch.zeros(n, PU.FRAME_FLOATS, device=DEV)
        cols[:, PU.FRAME_MPJPE] = d.mean(1)
        cols[:, PU.FRAME_PAMPJPE] = PU.pa_mpjpe_device(pred, gt)
        cols[:, PU.FRAME_PCK] = (d < 0.15).float().mean(1)
        cols[:, PU.FRAME_AUC] = (d[..., None] < thr).float().mean((1, 2))
        ap = pred[:-2] - 2 * pred[1:-1] + pred[2:]
        ag = gt[:-2] - 2 * gt[1:-1] + gt[2:]
        ok = (seq_id[:-2] == seq_id[2:]).float()
        cols[1:-1, PU.FRAME_ACCEL] = (ap - ag).norm(dim=-1).mean(1) * ok
        cols[1:-1, PU.FRAME_ACCEL_COUNTED] = ok
        sums = torch.zeros(S, PU.FRAME_FLOATS, device=DEV).index_add_(0, seq_id, cols)
        rows = torch.zeros(S, PU.SEQ_FLOATS, device=DEV)
        rows[:, PU.SEQ_FRAMES] = count
        rows[:, 1:5] = sums[:, :4] / count[:, None]
        rows[:, PU.SEQ_ACCEL] = sums[:, 4] / sums[:, 5].clamp(min=1)
        rows[:, PU.SEQ_TRIPLES] = sums[:, 5]
        return cols, rows

    legs = dict(kernel=kernel, torch=composed)
    for _ in range(o.warm):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(o.rounds):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            times[name].append(timed(fn)[0])
    (fk, sk), (ft, st) = kernel(), composed()
    torch.cuda.synchronize()
    fdiff = (fk - ft).abs().max(0).values.tolist()
    sdiff = (sk[:S] - st).abs().max(0).values.tolist()
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f"# {torch.cuda.get_device_name(0)}; {n} frames x {J} joints in {S} sequences of {min(lengths)} .. {max(lengths)} frames; "
          f"ms, median of {o.rounds} alternating rounds after {o.warm} warm-up calls (min .. max)")
    for k, v in times.items():
        print(f"{k:7s} {med[k]:8.3f} ({min(v):.3f} .. {max(v):.3f})")
    print(f"torch / kernel = {med['torch'] / med['kernel']:.2f}; per-frame columns max |diff| {['%.1e' % x for x in fdiff]}; "
          f"per-sequence columns max |diff| {['%.1e' % x for x in sdiff]}")
    print(json.dumps(dict(frames=n, sequences=S, joints=J, rounds=o.rounds, warm=o.warm,
                          **{k: dict(median_ms=round(med[k], 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4)) for k, v in times.items()},
                          frame_max_abs_diff=fdiff, seq_max_abs_diff=sdiff)))


if __name__ == "__main__":
    main()
