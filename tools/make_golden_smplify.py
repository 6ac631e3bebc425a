#!/usr/bin/env python3
"""Goldens of SMPLify: the REFERENCE's own ``utils/smplify`` code (imported read-only through the stub recipe of tools/make_golden.py)
over the oracle's LBS on the synthetic SMPL tables (``assets.make_synthetic_smpl(0)``; LBS itself stays unpinned, as elsewhere).
``SMPLify.__init__`` wants CUDA, ``config.SMPL_MODEL_DIR`` and ``human_body_prior``, so the object is made with ``object.__new__`` and
its fields are set here.

  tests/golden/g12_smplify_heads.npz   (a) ``camera_fitting_loss`` and ``body_fitting_loss`` on the seeded inputs: per-sample values,
                                       parts, the (B, 49) reprojection terms and autograd gradients w.r.t. joints, camera translation,
                                       body pose and betas - in fp32 and in fp64, the ignore mask off and on
  tests/golden/g12_smplify_fit.npz     (b) ``SMPLify.__call__`` at num_iters 0, 1 and 10 in fp32: inputs, the six outputs (vertices at
                                       every 23rd index), the per-sample loss of every iteration; (c) the same runs in fp64 - the
                                       noise floor -; the bounds per class of quantity (3 x the largest fp32-vs-fp64 difference,
                                       the convention of tools/make_noise.py); the margin data of the conditions below

The fp64 leg runs under ``torch.set_default_dtype(float64)`` (the reference's ``perspective_projection`` builds K with the default
dtype) and with the FLOAT32 prior tables upcast (``MaxMixturePrior(dtype=float32).to(float64)``: what assets/gmm_08_f32.npz holds) -
a prior built with dtype=float64 inverts the covariances in double and is a different function.

Inputs (B = 3, seeded): target poses N(0, 0.25) (global orientation halved), betas N(0, 0.5), camera depth 35 - 50; keypoints =
projection + 2 px noise, confidences in [0.2, 1]; initial values = target + noise of 0.15 / 0.3 / (0.05, 0.05, 3).  Sample 1 has two
of the four OpenPose torso confidences at 0 (the ground-truth-style torso is used), sample 2 a body joint at exactly (0, 0, 0),
sample 0 three non-ignored confidences at 0.

Conditions asserted here and re-asserted by tests/test_smplify_emu.py from the stored data (a seed that misses them is replaced,
never the condition):
  * the mixture component chosen is the same at every iteration in fp32 and fp64, and its gap to the runner-up is at least 100 x
    the fp32-vs-fp64 difference of the two values;
  * every optimised component's first-step gradient is at least 100 x its fp32-vs-fp64 difference.

usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_smplify.py [--out tests/golden] [--seed 1]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.dont_write_bytecode = True

import make_golden as MG                        # noqa: E402
from dynaboa_amd import assets                  # noqa: E402
from oracle import ref_cpu as O                 # noqa: E402

B = 3
FOCAL = 5000.0
ITERS = (0, 1, 10)
VERT_IDX = np.arange(0, 6890, 23)
IGN = ['OP Neck', 'OP RHip', 'OP LHip', 'Right Hip', 'Left Hip']
NOISE_FACTOR = 3.0
MARGIN = 100.0
F32, F64 = torch.float32, torch.float64


def make_inputs(seed, geo):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    true_pose = rn(B, 72) * 0.25
    true_pose[:, :3] *= 0.5
    true_betas = rn(B, 10) * 0.5
    true_t = torch.tensor([[0.05, -0.1, 40.0], [0.0, 0.1, 35.0], [-0.1, 0.0, 50.0]], dtype=F64)
    center = torch.full((B, 2), 112.0, dtype=F64)
    T64 = O.smpl_tables_to_torch(assets.make_synthetic_smpl(0), dtype=F64)
    _, j = O.smpl_forward(T64, true_betas, true_pose[:, 3:], true_pose[:, :3], pose2rot=True)
    torch.set_default_dtype(F64)
    proj = geo.perspective_projection(j, torch.eye(3, dtype=F64)[None].expand(B, -1, -1), true_t, FOCAL, center)
    torch.set_default_dtype(F32)
    assert 50.0 < float(proj.min()) and float(proj.max()) < 200.0, (float(proj.min()), float(proj.max()))
    conf = torch.rand(B, 49, 1, generator=g, dtype=F64) * 0.8 + 0.2
    conf[1, [9, 12]] = 0.0                      # sample 1: OpenPose hips invalid -> the ground-truth-style torso
    conf[0, [4, 20, 40]] = 0.0                  # sample 0: a few non-ignored joints without a detection
    kp = torch.cat([proj + rn(B, 49, 2) * 2.0, conf], -1)
    init_pose = true_pose + rn(B, 72) * 0.15
    init_pose[2, 3 + 3 * 5: 3 + 3 * 5 + 3] = 0.0  # sample 2: one body joint at exactly zero
    init_betas = true_betas + 0.3 * rn(B, 10)
    init_t = true_t + torch.tensor([0.05, 0.05, 3.0], dtype=F64)
    # everything the fp32 leg sees is an fp32 value; the fp64 leg sees the same values upcast
    q = lambda t: t.to(F32).to(F64)
    return dict(init_pose=q(init_pose), init_betas=q(init_betas), init_cam_t=q(init_t), center=q(center), kp=q(kp))


class Ref:
    def __init__(self):
        MG.install_stubs()
        os.chdir(MG.REF)
        import constants
        import utils.geometry as G
        import utils.smplify.prior as RP
        import utils.smplify.smplify as RS
        self.RS, self.RP, self.G, self.constants = RS, RP, G, constants
        self.tab = assets.make_synthetic_smpl(0)
        self.ign = [constants.JOINT_IDS[i] for i in IGN]

    def prior(self, dtype):
        torch.set_default_dtype(F32)
        p = self.RP.MaxMixturePrior(prior_folder=os.path.join(MG.REF, "data"), num_gaussians=8, dtype=F32).to(dtype)
        torch.set_default_dtype(dtype)
        return p

    def fitter(self, dtype, iters):
        s = object.__new__(self.RS.SMPLify)
        s.device, s.focal_length, s.step_size, s.num_iters = torch.device("cpu"), FOCAL, 1e-2, iters
        s.ign_joints = list(self.ign)
        s.pose_prior = self.prior(dtype)
        s.smpl = MG.SMPLStub(O.smpl_tables_to_torch(self.tab, dtype=dtype))
        return s

    def run(self, inp, dtype, iters):
        """-> outputs (6 tensors), record: per-sample loss of every iteration, the mixture's (best, second, argmin) at every body
        iteration, the gradients each optimiser step applied."""
        RS = self.RS
        s = self.fitter(dtype, iters)
        rec = dict(loss=[], gmm=[], grads=[])
        cam0, body0, step0 = RS.camera_fitting_loss, RS.body_fitting_loss, torch.optim.Adam.step

        def cam(model_joints, camera_t, est, center, j2d, conf, **k):
            with torch.no_grad():
                rec["loss"].append(torch.stack([cam0(model_joints[i:i + 1], camera_t[i:i + 1], est[i:i + 1], center[i:i + 1], j2d[i:i + 1],
                                                     conf[i:i + 1], **k) for i in range(B)]))
            return cam0(model_joints, camera_t, est, center, j2d, conf, **k)

        def body(body_pose, betas, model_joints, camera_t, center, j2d, conf, prior, **k):
            if k.get("output", "sum") == "sum":
                with torch.no_grad():
                    rec["loss"].append(torch.stack([body0(body_pose[i:i + 1], betas[i:i + 1], model_joints[i:i + 1], camera_t[i:i + 1],
                                                          center[i:i + 1], j2d[i:i + 1], conf[i:i + 1], prior, **k) for i in range(B)]))
                    d = body_pose[:, None, :] - prior.means
                    q = 0.5 * torch.einsum('bmi,mij,bmj->bm', d, prior.precisions, d) - torch.log(prior.nll_weights)
                    sq, order = q.sort(1)
                    rec["gmm"].append(torch.stack([sq[:, 0], sq[:, 1], order[:, 0].to(q.dtype)], 1))
            return body0(body_pose, betas, model_joints, camera_t, center, j2d, conf, prior, **k)

        def step(opt, *a, **k):
            rec["grads"].append(torch.cat([p.grad.detach().reshape(B, -1) for grp in opt.param_groups for p in grp["params"]], 1).clone())
            return step0(opt, *a, **k)

        RS.camera_fitting_loss, RS.body_fitting_loss, torch.optim.Adam.step = cam, body, step
        try:
            c = lambda k: inp[k].to(dtype).clone()
            out = s(c("init_pose"), c("init_betas"), c("init_cam_t"), c("center"), c("kp"))
        finally:
            RS.camera_fitting_loss, RS.body_fitting_loss, torch.optim.Adam.step = cam0, body0, step0
        torch.set_default_dtype(F32)
        return [x.detach().double() for x in out], rec


NAMES = ["vertices", "joints", "pose", "betas", "cam_t", "reproj"]


def fit_golden(ref, inp):
    P = {k: v.numpy().astype(np.float32) for k, v in inp.items()}
    P["vert_idx"], P["iters"] = VERT_IDX.astype(np.int32), np.array(ITERS, np.int32)
    floors = {n: 0.0 for n in NAMES + ["loss_cam", "loss_body"]}
    for it in ITERS:
        (o32, r32), (o64, r64) = ref.run(inp, F32, it), ref.run(inp, F64, it)
        for n, a, b in zip(NAMES, o32, o64):
            a, b = a.numpy(), b.numpy()
            if n == "vertices":
                a, b = a[:, VERT_IDX], b[:, VERT_IDX]
            P[f"i{it}_{n}_f32"], P[f"i{it}_{n}_f64"] = a.astype(np.float32), b
            floors[n] = max(floors[n], float(np.abs(a - b).max()))
        if it:
            l32, l64 = torch.stack(r32["loss"]).double().numpy(), torch.stack(r64["loss"]).double().numpy()
            P[f"i{it}_loss_f32"], P[f"i{it}_loss_f64"] = l32.astype(np.float32), l64
            floors["loss_cam"] = max(floors["loss_cam"], float(np.abs(l32[:it] - l64[:it]).max()))
            floors["loss_body"] = max(floors["loss_body"], float(np.abs(l32[it:] - l64[it:]).max()))
            g32, g64 = torch.stack(r32["gmm"]).double().numpy(), torch.stack(r64["gmm"]).double().numpy()
            P[f"i{it}_gmm_f32"], P[f"i{it}_gmm_f64"] = g32, g64              # [iter][B][best, second, component]
            # the gradients of the first step of each stage: stage 1 (global orientation 3 | camera 3), stage 2 (body 69 | betas 10 | orientation 3)
            for tag, k in (("s1", 0), ("s2", it)):
                P[f"i{it}_g{tag}_f32"], P[f"i{it}_g{tag}_f64"] = r32["grads"][k].double().numpy(), r64["grads"][k].double().numpy()
    for n, v in floors.items():
        P[f"floor_{n}"], P[f"bound_{n}"] = np.float64(v), np.float64(NOISE_FACTOR * v)
    check_margins(P)
    return P


def check_margins(P):
    """The conditions of the module docstring, from the stored arrays alone (tests/smplify_cases.py re-asserts them)."""
    worst = dict(gap=np.inf, grad=np.inf)
    for it in [int(i) for i in P["iters"] if int(i) > 0]:
        g32, g64 = P[f"i{it}_gmm_f32"], P[f"i{it}_gmm_f64"]
        assert np.array_equal(g32[..., 2], g64[..., 2]), ("mixture component differs between fp32 and fp64", it)
        assert np.all(g64[..., 2] == g64[:1, :, 2]), ("mixture component changes during the fit", it)
        gap = g64[..., 1] - g64[..., 0]
        diff = np.maximum(np.abs(g32[..., 0] - g64[..., 0]), np.abs(g32[..., 1] - g64[..., 1]))
        ratio = float((gap / np.maximum(diff, 1e-300)).min())
        assert ratio >= MARGIN, ("mixture gap below %g x the fp32-vs-fp64 difference" % MARGIN, it, ratio)
        worst["gap"] = min(worst["gap"], ratio)
        for tag in ("s1", "s2"):
            a, b = P[f"i{it}_g{tag}_f32"], P[f"i{it}_g{tag}_f64"]
            r = float((np.abs(b) / np.maximum(np.abs(a - b), 1e-300)).min())
            assert r >= MARGIN, ("a first-step gradient below %g x its fp32-vs-fp64 difference" % MARGIN, it, tag, r)
            worst["grad"] = min(worst["grad"], r)
    return worst


def heads_golden(ref, inp):
    """(a): the two loss functions at the initial values (camera moved off its estimate so that the depth term is live)."""
    RSL = sys.modules["utils.smplify.losses"]
    P = {k: v.numpy().astype(np.float32) for k, v in inp.items()}
    off = torch.tensor([0.01, -0.02, 0.5], dtype=F64)
    floors = {}
    for dtype, tag in ((F32, "f32"), (F64, "f64")):
        prior = ref.prior(dtype)
        T = O.smpl_tables_to_torch(ref.tab, dtype=dtype)
        c = lambda k: inp[k].to(dtype).clone()
        pose, kp, center, est = c("init_pose"), c("kp"), c("center"), c("init_cam_t")
        with torch.no_grad():
            _, joints = O.smpl_forward(T, c("init_betas"), pose[:, 3:], pose[:, :3], pose2rot=True)
        if dtype == F32:
            P["joints"] = joints.numpy().copy()
            P["cam_t"] = (est + off.to(dtype)).numpy().copy()
        joints = torch.from_numpy(P["joints"]).to(dtype).requires_grad_(True)      # both legs differentiate at the same fp32 points
        cam_t = torch.from_numpy(P["cam_t"]).to(dtype).requires_grad_(True)
        bp, be = pose[:, 3:].clone().requires_grad_(True), c("init_betas").requires_grad_(True)
        R = {}
        per = torch.stack([RSL.camera_fitting_loss(joints[i:i + 1], cam_t[i:i + 1], est[i:i + 1], center[i:i + 1], kp[i:i + 1, :, :2],
                                                   kp[i:i + 1, :, 2], focal_length=FOCAL) for i in range(B)])
        tot = RSL.camera_fitting_loss(joints, cam_t, est, center, kp[:, :, :2], kp[:, :, 2], focal_length=FOCAL)
        R["cam_loss"], (R["cam_djoints"], R["cam_dcam_t"]) = per.detach(), torch.autograd.grad(tot, [joints, cam_t])
        for ign in (0, 1):
            conf = kp[:, :, 2].clone()
            if ign:
                conf[:, ref.ign] = 0.0
            a = (joints, cam_t, center, kp[:, :, :2], conf, prior)
            per = torch.stack([RSL.body_fitting_loss(bp[i:i + 1], be[i:i + 1], joints[i:i + 1], cam_t[i:i + 1], center[i:i + 1], kp[i:i + 1, :, :2],
                                                     conf[i:i + 1], prior, focal_length=FOCAL) for i in range(B)])
            tot = RSL.body_fitting_loss(bp, be, *a, focal_length=FOCAL)
            gr = torch.autograd.grad(tot, [bp, be, joints, cam_t])
            rp = RSL.body_fitting_loss(bp, be, *a, focal_length=FOCAL, output='reprojection').detach()
            parts = torch.stack([rp.sum(-1), (4.78 ** 2) * prior(bp, be).detach(), (15.2 ** 2) * RSL.angle_prior(bp).sum(-1).detach(),
                                 (5 ** 2) * (be.detach() ** 2).sum(-1), per.detach()], 1)
            k = f"body{ign}"
            R[k + "_parts"], R[k + "_reproj"] = parts, rp
            R[k + "_dpose"], R[k + "_dbetas"], R[k + "_djoints"], R[k + "_dcam_t"] = gr
        torch.set_default_dtype(F32)
        for k, v in R.items():
            v = v.detach().double().numpy()
            P[f"{k}_{tag}"] = v.astype(np.float32) if tag == "f32" else v
    for k in [k[:-4] for k in P if k.endswith("_f64")]:
        v = float(np.abs(P[k + "_f32"].astype(np.float64) - P[k + "_f64"]).max())
        P[f"floor_{k}"], P[f"bound_{k}"] = np.float64(v), np.float64(NOISE_FACTOR * v)
    return P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    out = os.path.abspath(a.out)
    torch.set_num_threads(1)                    # one summation order, whatever the machine: the files regenerate bit for bit
    torch.manual_seed(0)
    ref = Ref()
    inp = make_inputs(a.seed, ref.G)
    heads = heads_golden(ref, inp)
    np.savez_compressed(os.path.join(out, "g12_smplify_heads.npz"), **heads)
    fit = fit_golden(ref, inp)
    fit["seed"] = np.int32(a.seed)
    np.savez_compressed(os.path.join(out, "g12_smplify_fit.npz"), **fit)
    for k in sorted(k for k in list(fit) + list(heads) if k.startswith("floor_")):
        print("%-28s floor %.3e" % (k[6:], float((fit if k in fit else heads)[k])))
    print("margins (>= %g): %s" % (MARGIN, check_margins(fit)))
    for f in ("g12_smplify_heads.npz", "g12_smplify_fit.npz"):
        print(f, os.path.getsize(os.path.join(out, f)), "bytes")


if __name__ == "__main__":
    main()
