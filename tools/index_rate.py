#!/usr/bin/env python3
"""Time per Lloyd iteration of the retrieval-index k-means (dynaboa_amd/retrieval_index.py, csrc/kmeans.hip), split into assign and
update, on synthetic features: N = 100 000 and 300 000 rows of D = 2048 (Human3.6M at every 5th frame of one camera is of that
order), K = 10 and 100 centres.  Each time is set against two comparison objects measured in the same process:

  floor   the HBM floor of TWO reads of the feature matrix per iteration (one by the assign, one by the update) at the achievable
          streaming bandwidth DESIGN.md uses (5.2 TB/s): N * D * 4 bytes / 5.2e12 per step
  torch   the plain torch composition on the device: ``(X @ Cn.T).argmax(1)`` for the assign (an [N][K] intermediate),
          ``zeros(K, D).index_add_(0, assign, Xn) / counts`` for the update (floating-point atomics: not deterministic); Xn, the
          normalised copy of X, is made once outside the clock (a second N x D matrix the kernels do not need)

Device events around each step, every shape warmed up, the legs alternating inside each of --rounds rounds, medians reported with the
spread.  The assignments of the two forms are compared on the same inputs (rows that differ are counted; random centres leave some
rows undecided up to rounding).  One JSON line per shape.

usage:  timeout 600 python tools/index_rate.py [--rows 100000,300000] [--clusters 10,100] [--rounds 7] [--warm 3]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dynaboa_amd import retrieval_index as RI      # noqa: E402

DEV = "cuda:0"
D = 2048
HBM = 5.2e12                                        # bytes / s (what the streaming optimiser kernels reach)


def features(N, K, seed):
    """K blobs with noise as large as the signal: rows in the same blob have cosine ~ 0.5, an iteration moves real members"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    dirs = torch.randn(K, D, device=DEV, generator=g)
    blob = torch.randint(0, K, (N,), device=DEV, generator=g)
    x = torch.empty(N, D, device=DEV)
    for lo in range(0, N, 50000):
        hi = min(N, lo + 50000)
        x[lo:hi] = (dirs[blob[lo:hi]] + torch.randn(hi - lo, D, device=DEV, generator=g)) * (0.5 + 2.5 * torch.rand(hi - lo, 1, device=DEV, generator=g))
    return x


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", default="100000,300000")
    p.add_argument("--clusters", default="10,100")
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--warm", type=int, default=3)
    o = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("index_rate: needs the GPU (no fall-back: a CPU time says nothing about the device)")
    print(f"# {torch.cuda.get_device_name(0)}; D = {D}; floor = N * D * 4 B / {HBM / 1e12:.1f} TB/s per step; ms, median of {o.rounds} rounds (min .. max)")
    for N in [int(v) for v in o.rows.split(",")]:
        for K in [int(v) for v in o.clusters.split(",")]:
            x = features(N, K, 1000 + K)
            ops = RI._torch_ops(x, K)
            rows = torch.tensor(RI.init_rows(N, K, 22), device=DEV)
            ops.start(x[rows].cpu().numpy())
            xn = torch.nn.functional.normalize(x, dim=1, eps=1e-8)
            state = {}

            def ours_assign():
                state["small"] = ops.assign_step()          # centre norms + assign + the iteration's one small read

            def ours_update():
                ops.update(state["small"][1])

            def torch_assign():
                cn = torch.nn.functional.normalize(ops.centers, dim=1, eps=1e-8)
                state["t_assign"] = (xn @ cn.T).argmax(1)
                state["t_counts"] = torch.bincount(state["t_assign"], minlength=K)
                state["t_counts_host"] = state["t_counts"].cpu()            # the loop's stop test needs them on the host too

            def torch_update():
                sums = torch.zeros(K, D, device=DEV).index_add_(0, state["t_assign"], xn)
                state["t_centers"] = sums / state["t_counts"].clamp(min=1)[:, None]

            legs = dict(assign=ours_assign, update=ours_update, torch_assign=torch_assign, torch_update=torch_update)
            # two real iterations first so that the timed state is a mid-run one, then the warm-up of every leg
            for _ in range(2):
                ours_assign()
                ours_update()
            for _ in range(o.warm):
                for fn in legs.values():
                    fn()
            torch.cuda.synchronize()
            centres0 = ops.centers.clone()
            times = {k: [] for k in legs}
            for _ in range(o.rounds):
                for name, fn in legs.items():                                # alternating; the centres are the same for every round
                    ops.centers.copy_(centres0)
                    torch.cuda.synchronize()
                    times[name].append(timed(fn)[0])
            ops.centers.copy_(centres0)
            ours_assign()
            torch_assign()
            differ = int((ops.assign.long() != state["t_assign"]).sum())
            ours_update()
            torch_update()
            nz = state["t_counts"] > 0
            cdiff = float((ops.centers[nz] - state["t_centers"][nz]).abs().max())
            floor = N * D * 4 / HBM * 1e3
            med = {k: statistics.median(v) for k, v in times.items()}
            rec = dict(N=N, K=K, D=D, rounds=o.rounds, floor_ms_per_step=round(floor, 4), assign_rows_that_differ=differ,
                       centres_max_abs_diff=cdiff,
                       **{k: dict(median_ms=round(med[k], 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4)) for k, v in times.items()})
            print(f"N {N:7d} K {K:4d} | floor/step {floor:6.3f} | assign {med['assign']:7.3f} ({min(times['assign']):.3f} .. {max(times['assign']):.3f})"
                  f"  torch {med['torch_assign']:7.3f} ({min(times['torch_assign']):.3f} .. {max(times['torch_assign']):.3f})"
                  f" | update {med['update']:7.3f} ({min(times['update']):.3f} .. {max(times['update']):.3f})"
                  f"  torch {med['torch_update']:7.3f} ({min(times['torch_update']):.3f} .. {max(times['torch_update']):.3f})"
                  f" | iteration {med['assign'] + med['update']:7.3f} vs torch {med['torch_assign'] + med['torch_update']:7.3f} vs floor {2 * floor:6.3f}"
                  f" | rows that differ {differ}, centres max |diff| {cdiff:.2e}")
            print(json.dumps(rec))
            del x, xn, ops, state
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
