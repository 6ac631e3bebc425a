#!/usr/bin/env python3
"""Golden of the sequence metrics: the REFERENCE's own ``utils/pose_utils.py`` (imported read-only by path; it needs NumPy alone) on the
seeded ragged batches of tests/seq_metrics_cases.py (J = 14 and J = 17; sequence lengths 1, 2, 3, 0, 64, 65, 130), fed as float64
copies of the fp32 inputs - the arithmetic the kernel's bounds are derived for.

  tests/golden/g14_seq_metrics.npz   pred<J>, gt<J>     the inputs, fp32 [265][J][3] (the tests regenerate them and compare)
                                     lengths, vis        the sequence lengths; `vis` with one invisible frame inside the 65-frame sequence
                                     re<J> pck<J> auc<J> reconstruction_error(needpck=True, needauc=True) of every SINGLE sample (the
                                                         reference's compute_pck raises from the second sample on)
                                     accel<J>_s<k>       compute_error_accel(gt, pred) of sequence k (those with >= 3 frames)
                                     accel_vis<J>_s<k>   the same with vis
Data only.  The generator asserts that no joint distance of the file lies within 1e-6 of the PCK threshold or of an AUC threshold,
so that no rounding can decide a PCK.

usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_seq_metrics.py [--reference /root/reference]
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

import seq_metrics_cases as SC                  # noqa: E402


def reference_module(root):
    spec = importlib.util.spec_from_file_location("ref_pose_utils", os.path.join(root, "utils", "pose_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g14_seq_metrics.npz"))
    o = ap.parse_args()
    R = reference_module(o.reference)
    # the reference's defaults are what the tests pass to the kernel
    assert np.array_equal(SC.THRESHOLDS, np.linspace(0, 150, 31) / 1000) and SC.PCK_THR == 0.15
    out = dict(lengths=np.asarray(SC.LENGTHS, np.int32), vis=SC.vis_mid())
    off = SC.offsets_of(SC.LENGTHS)
    for J in SC.JOINTS:
        pred, gt = SC.make_batch(J)
        gap = SC.margin(pred, gt)
        assert gap >= SC.MARGIN, (J, gap)
        p, g = pred.astype(np.float64), gt.astype(np.float64)
        rows = [R.reconstruction_error(p[i:i + 1], g[i:i + 1], needpck=True, needauc=True, reduction=None) for i in range(len(p))]
        out[f"pred{J}"], out[f"gt{J}"] = pred, gt
        out[f"re{J}"] = np.array([float(r[0][0]) for r in rows])
        out[f"pck{J}"] = np.array([float(r[1][0]) for r in rows])
        out[f"auc{J}"] = np.array([float(r[2]) for r in rows])
        for s, n in enumerate(SC.LENGTHS):
            if n >= 3:
                a, b = off[s], off[s + 1]
                out[f"accel{J}_s{s}"] = R.compute_error_accel(g[a:b], p[a:b])
                out[f"accel_vis{J}_s{s}"] = R.compute_error_accel(g[a:b], p[a:b], out["vis"][a:b].astype(bool))
        print(f"J {J}: {len(p)} frames, margin {gap:.3e}, PA-MPJPE {out[f're{J}'].mean():.4f}, PCK {out[f'pck{J}'].mean():.3f}, AUC {out[f'auc{J}'].mean():.3f}")
    np.savez_compressed(o.out, **out)
    print(o.out, os.path.getsize(o.out), "bytes")


if __name__ == "__main__":
    main()
