#!/usr/bin/env python3
"""What the device-resident exemplar bank (``--exemplar_bank 1``; dynaboa_amd/exemplar_bank.py, csrc/retrieval.hip) is worth on a real
data tree.  Writes a reference-style tree from seeds (SMPL pickles, checkpoint, pose prior, a 3DPW-format stream, E exemplars in K
clusters), then steps the reference's default term set WITHOUT a synthetic bundle at S = 1, 8, 32 sequences per GPU, four legs
interleaved in one process:

  callback   --exemplar_bank 0: the retrieval callback of the native stepper - per level and sequence a stream synchronise, an
             ``.item()``, ``random.sample``, a PNG decode + crop and five uploads; parallel passes off (the code path of the parent
             commit, which this flag leaves untouched)
  bank_seq   --exemplar_bank 1 with ``par_passes`` 0: select + gather kernels in line
  bank       --exemplar_bank 1 at its defaults: history and exemplar passes beside the frame pass
  bundle     the synthetic bundle with the same flags (exemplars handed over up front): the ceiling

The stream's frames are decoded and cropped before the clock starts (the same tensors for every leg); what the callback route does per
level is inside it.  One JSON line per (S, leg) with every repetition's frames per second.

usage:  timeout 900 python tools/retrieval_rate.py [--seqs 1,8,32] [--frames 12] [--warm 3] [--reps 2] [--exemplars 240] [--clusters 24]
"""
import argparse
import json
import os
import pickle
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dynaboa_amd import assets, benchmark as DB, datasets as D, native_step as NS      # noqa: E402
from dynaboa_amd.base_adaptor import synthetic_bundle                                   # noqa: E402

DEV = "cuda:0"


def write_tree(root, nseq, nframes, exemplars, clusters):
    """data/{smpl, spin_data, dataset_extras, retrieval_res}, basemodel.pt, the stream's and the exemplars' PNGs - the formats of the
    reference's files, content from seeds."""
    import joblib
    import scipy.sparse as sp
    from PIL import Image
    rng = np.random.default_rng(5)
    data = os.path.join(root, "data")
    for d in ("smpl", "spin_data", "dataset_extras", "retrieval_res"):
        os.makedirs(os.path.join(data, d))
    tabs = {g: assets.make_synthetic_smpl(i) for i, g in enumerate(("NEUTRAL", "MALE", "FEMALE"))}
    for g, t in tabs.items():
        V = t["v_template"].shape[0]
        kin = np.stack([np.asarray(t["parents"]).astype(np.int64) % (2 ** 32), np.arange(24)]).astype(np.uint32)
        d = dict(v_template=t["v_template"].astype(np.float64),
                 shapedirs=np.concatenate([t["shapedirs"].astype(np.float64), rng.normal(0, 0.01, (V, 3, 290))], 2),
                 posedirs=t["posedirs"].T.reshape(V, 3, 207).astype(np.float64), J_regressor=sp.csc_matrix(t["J_regressor"].astype(np.float64)),
                 weights=t["lbs_weights"].astype(np.float64), kintree_table=kin, f=t["faces"].astype(np.uint32), bs_type="lrotmin", bs_style="lbs")
        with open(os.path.join(data, "smpl", f"SMPL_{g}.pkl"), "wb") as f:
            pickle.dump(d, f, protocol=2)
    np.save(os.path.join(data, "J_regressor_extra.npy"), tabs["NEUTRAL"]["J_regressor_extra"])
    np.save(os.path.join(data, "J_regressor_h36m.npy"), tabs["NEUTRAL"]["J_regressor_h36m"])
    mp = assets.make_smpl_mean_params(identity_pose=False, seed=3)
    np.savez(os.path.join(data, "smpl_mean_params.npz"), **mp)
    torch.save(assets.make_synthetic_checkpoint(22, mp, randomize_norm=True, prefix="module."), os.path.join(data, "basemodel.pt"))
    covs = []
    for _ in range(8):
        a = rng.normal(0, 1, (69, 69))
        covs.append(a @ a.T / 69 + 0.5 * np.eye(69))
    with open(os.path.join(data, "spin_data", "gmm_08.pkl"), "wb") as f:
        pickle.dump(dict(means=rng.normal(0, 0.3, (8, 69)), covars=np.stack(covs), weights=np.full(8, 0.125)), f, protocol=2)

    def png(path, h, w):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(path)
    imgroot, h36root = os.path.join(root, "pw3d_images"), os.path.join(root, "h36m_images")
    for s in range(nseq):
        names = []
        for i in range(nframes):
            names.append(f"imageFiles/seq{s}/image_{i:05d}.png")
            png(os.path.join(imgroot, names[-1]), 96, 128)
        n = nframes
        np.savez(os.path.join(data, "dataset_extras", f"3dpw_{s}_0.npz"), imgname=np.array(names), scale=rng.uniform(0.3, 0.7, n),
                 center=rng.uniform(30, 90, (n, 2)), pose=rng.normal(0, 0.2, (n, 72)), shape=rng.normal(0, 0.5, (n, 10)),
                 j2d=np.concatenate([rng.uniform(0, 120, (n, 49, 2)), (rng.random((n, 49, 1)) < 0.8).astype(float)], 2),
                 op_j2d=np.concatenate([rng.uniform(0, 120, (n, 25, 2)), rng.random((n, 25, 1))], 2), gender=np.array(["m"] * n))
    M = exemplars
    names = []
    for i in range(M):
        names.append(f"S1/img_{i:05d}.png")
        png(os.path.join(h36root, names[-1]), 96, 96)
    rr = os.path.join(data, "retrieval_res")
    joblib.dump(dict(imgname=np.array(names), scale=rng.uniform(0.25, 0.45, M), center=rng.uniform(35, 60, (M, 2)), pose=rng.normal(0, 0.2, (M, 72)),
                     shape=rng.normal(0, 0.5, (M, 10)), S=np.concatenate([rng.normal(0, 0.3, (M, 24, 3)), np.ones((M, 24, 1))], 2),
                     part=np.concatenate([rng.uniform(0, 96, (M, 24, 2)), (rng.random((M, 24, 1)) < 0.8).astype(float)], 2)),
                os.path.join(rr, "h36m_random_sample_center_10_10.pt"))
    index = [[int(i) for i in range(M) if i % clusters == k] for k in range(clusters)]
    joblib.dump(dict(centers=rng.normal(0, 1, (clusters, 2048)).astype(np.float32), index=index),
                os.path.join(rr, "cluster_res_random_sample_center_10_10_potocol2.pt"))
    return imgroot, h36root


LEGS = ("callback", "bank_seq", "bank", "bundle")


def make_adaptors(leg, S, base):
    import copy
    os.environ["DYB_PAR_PASSES"] = "0" if leg == "bank_seq" else "1"
    ads = []
    bundle = synthetic_bundle(seed=22, identity_pose=False, randomize_norm=True, smpl_seed=0) if leg == "bundle" else None
    for _ in range(S):
        o = copy.copy(base)
        o.exemplar_bank = 1 if leg in ("bank_seq", "bank") else 0
        ads.append(DB.Adaptor(o, bundle, device=DEV))
    return ads


def run_leg(leg, S, base, frames, warm):
    """frames[r][step]: the collated batches of sequence r -> frames per second over the steps after `warm`"""
    ads = make_adaptors(leg, S, base)
    nsteps = len(frames[0])
    if S == 1:
        ad = ads[0]
        ad.reset_records(nsteps)
    else:
        grp = NS.ReplicaGroup(ads, nsteps)
    for step in range(nsteps):
        if step == warm:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        if S == 1:
            ad.global_step = step
            ad.fit_losses = {}
            ad.model.eval()
            ad.adaptation(frames[0][step])
        else:
            grp.step([frames[r][step] for r in range(S)], step)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ns = ads[0]._native
    assert ns is not None and ns.full
    info = dict(callback=ns._cb is not None, draws=[int(getattr(a, "_bank_draw", 0)) for a in ads[:2]],
                extra_steps=[int(sum(a.optim_step_record)) for a in ads[:2]])
    return S * (nsteps - warm) / dt, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", default="1,8,32")
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--exemplars", type=int, default=240)
    ap.add_argument("--clusters", type=int, default=24)
    ap.add_argument("--legs", default=",".join(LEGS))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("retrieval_rate.py measures on the GPU; there is none")
    seqs = [int(x) for x in a.seqs.split(",")]
    legs = [x for x in a.legs.split(",") if x in LEGS]
    NS.set_replica_policy(True)
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        imgroot, h36root = write_tree(root, max(seqs), a.frames, a.exemplars, a.clusters)
        os.chdir(root)
        base = DB.parser.parse_args(["--model_file", "data/basemodel.pt", "--expdir", os.path.join(root, "exps"), "--deferred_metrics", "1"])
        base.pw3d_root, base.h36m_root = imgroot, h36root
        ds = D.PW3D(None, img_dir=imgroot, device=DEV)
        frames = [[D.collate([ds[s["first"] + i]]) for i in range(s["frames"])] for s in ds.sequences]
        print(json.dumps(dict(tree=dict(sequences=len(frames), frames=a.frames, exemplars=a.exemplars, clusters=a.clusters),
                              bank_mb=round(a.exemplars * 603412 / 2 ** 20, 1), setup_s=round(time.perf_counter() - t0, 1))), flush=True)
        for S in seqs:
            fps = {leg: [] for leg in legs}
            info = {}
            for _ in range(a.reps):                       # the legs alternate inside one process and session
                for leg in legs:
                    f, info[leg] = run_leg(leg, S, base, frames, a.warm)
                    fps[leg].append(round(f, 2))
            for leg in legs:
                v = fps[leg]
                print(json.dumps(dict(seqs=S, leg=leg, frames_per_s=v, best=max(v), spread=round(max(v) - min(v), 2), **info[leg])), flush=True)


if __name__ == "__main__":
    main()
