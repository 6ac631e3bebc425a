"""Cases of the SMPLify kernels (csrc/smplify.hip) and of the one-call fit, shared by tests/test_smplify_emu.py (host build of the
kernels) and tests/test_smplify_gpu.py (MI355X).  References: fp64 autograd of oracle.ref_cpu.smplx_rodrigues, torch.optim.Adam on
the CPU, and the goldens g12_smplify_* (tools/make_golden_smplify.py: the reference's own utils/smplify code in fp32 and in fp64).

Bounds.  Everything held against a golden is compared with the reference's FP64 record, within the bound stored next to it: 3 x the
largest fp32-vs-fp64 difference the reference itself shows over the class of quantity (the convention of tools/make_noise.py); no
bound here comes from this project's output.  The two cases without a golden state their own reasoning (RODRIGUES_TOL, ADAM_TOL)."""
import numpy as np
import torch

from kernel_cases import smpl_device_tables
from oracle import ref_cpu as O

# dyb_rodrigues_bwd against fp64 autograd: about thirty fp32 operations (each <= 1 ulp, sinf / cosf <= 2), every intermediate O(1) x
# the incoming gradient once c1 is formed as 2 sin^2(a / 2) and the radial term is multiplied by e ~ a again - under 100 ulp = 6e-6
# of the row's scale.  1e-5 of max(1, largest reference component of the row).
RODRIGUES_TOL = 1e-5
# dyb_smplify_adam against torch.optim.Adam (fp32, CPU): the same formula in the same order; per step the parameter rounds once
# (1 ulp of |p| < 2: 2.4e-7) and the update lr * m / denom carries a few ulp of relative error (< 1e-5 * lr = 1e-7).  Three steps:
# 1e-6 absolute.  Moments: 1e-5 relative to the largest moment of the group (a few ulp per step).
ADAM_TOL = 1e-6
ADAM_MOMENT_TOL = 1e-5
MARGIN = 100.0


def _check(rc, what):
    assert rc == 0, (what, rc)


def gmm_dev(be, gmm):
    with np.errstate(divide="ignore"):                                  # -inf for an underflowed weight, as torch.log gives
        logw = np.log(gmm["nll_weights"]).astype(np.float32).reshape(-1)
    return be.dev(gmm["means"]), be.dev(gmm["precisions"]), be.dev(logw)


# ---------------------------------------------------------------------------------------- rodrigues backward
def rodrigues_inputs(n, seed=3):
    rng = np.random.default_rng(seed)
    aa = (rng.standard_normal((n, 3)) * 0.8).astype(np.float32)
    unit = lambda v: np.asarray(v, np.float64) / np.linalg.norm(v)
    aa[0] = 0.0                                                         # the exact zero vector: where the reference starts body poses
    if n >= 3:
        aa[n - 1] = (unit([0.3, -0.5, 0.8]) * 1e-4).astype(np.float32)            # an angle of 1e-4
        aa[n - 2] = (unit([-0.6, 0.2, 0.7]) * (np.pi - 1e-3)).astype(np.float32)  # an angle near pi
    dR = rng.standard_normal((n, 3, 3)).astype(np.float32)
    return aa, dR


def case_rodrigues_bwd(be, n):
    aa, dR = rodrigues_inputs(n)
    x = torch.from_numpy(aa).double().requires_grad_(True)
    (ref,) = torch.autograd.grad((O.smplx_rodrigues(x) * torch.from_numpy(dR).double()).sum(), x)
    ref = ref.numpy()
    assert np.isfinite(ref).all()
    out = be.empty((n, 3))
    _check(be.lib.dyb_rodrigues_bwd(be.ptr(be.dev(aa)), be.ptr(be.dev(dR)), be.ptr(out), n, be.stream), "rodrigues bwd")
    got = be.host(out).astype(np.float64)
    assert np.isfinite(got).all()
    err = np.abs(got - ref).max(axis=1) / np.maximum(1.0, np.abs(ref).max(axis=1))
    print("rodrigues bwd n=%d worst row %d err %.2e (zero row %.2e)" % (n, int(err.argmax()), err.max(), err[0]))
    assert err.max() < RODRIGUES_TOL, (int(err.argmax()), err.max())
    # at r = 0 the gradient is the generators' contraction (sin a / a = 1): (G21 - G12, G02 - G20, G10 - G01)
    w = np.array([dR[0, 2, 1] - dR[0, 1, 2], dR[0, 0, 2] - dR[0, 2, 0], dR[0, 1, 0] - dR[0, 0, 1]], np.float64)
    assert np.abs(ref[0] - w).max() < 1e-6 and np.abs(got[0] - w).max() < RODRIGUES_TOL * max(1.0, np.abs(w).max())
    return float(err.max())


# ---------------------------------------------------------------------------------------- loss heads against golden (a)
def _within(name, got, ref64, bound, errs):
    e = float(np.abs(np.asarray(got, np.float64) - ref64).max())
    errs[name] = (e, float(bound))
    return e <= float(bound)


def _report(what, errs):
    print(what, {k: "%.2e / %.2e" % v for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v[0] <= v[1]}
    assert not bad, (what, "beyond 3 x the reference's fp32-vs-fp64 floor (error, bound)", bad)


def case_camera_loss(be, g, sel):
    """dyb_smplify_camera_loss on the samples `sel` of golden (a): sample 1 takes the ground-truth-style torso, the others the OpenPose one."""
    sel, n = list(sel), len(sel)
    D = lambda k: be.dev(g[k][sel])
    loss, dj, dc = be.empty((n,)), be.empty((n, 49, 3)), be.empty((n, 3))
    _check(be.lib.dyb_smplify_camera_loss(be.ptr(D("joints")), be.ptr(D("cam_t")), be.ptr(D("init_cam_t")), be.ptr(D("center")), be.ptr(D("kp")),
                                          5000.0, 100.0, be.ptr(loss), be.ptr(dj), be.ptr(dc), n, be.stream), "camera loss")
    errs = {}
    for name, got in (("cam_loss", loss), ("cam_djoints", dj), ("cam_dcam_t", dc)):
        _within(name, be.host(got), g[name + "_f64"][sel].reshape(be.host(got).shape), g["bound_" + name], errs)
    _report("camera loss %s" % sel, errs)
    djh = be.host(dj)
    for i, s in enumerate(sel):                    # the branch: exactly the four selected joints carry a gradient
        live = sorted(np.nonzero(np.abs(djh[i]).max(axis=1) > 0)[0].tolist())
        assert live == ([27, 28, 33, 34] if s == 1 else [2, 5, 9, 12]), (s, live)
    return errs


def case_body_loss(be, g, gmm, sel, ignore):
    sel, n = list(sel), len(sel)
    D = lambda k: be.dev(g[k][sel])
    G = gmm_dev(be, gmm)
    pose = be.dev(g["init_pose"][sel])                     # [n][72]: the body pose is read in place, leading dimension 72
    parts, reproj, tot = be.empty((n, 5)), be.empty((n, 49)), be.empty((n,))
    dj, dp, db, dc = be.empty((n, 49, 3)), be.empty((n, 69)), be.empty((n, 10)), be.empty((n, 3))
    kp = D("kp")
    kp_before = be.host(kp).copy()
    _check(be.lib.dyb_smplify_body_loss(be.ptr(pose) + 12, 72, be.ptr(D("init_betas")), 10, be.ptr(D("joints")), be.ptr(D("cam_t")),
                                        be.ptr(D("center")), be.ptr(kp), be.ptr(G[0]), be.ptr(G[1]), be.ptr(G[2]), 5000.0, 100.0, 4.78, 5.0, 15.2,
                                        int(ignore), be.ptr(parts), be.ptr(reproj), be.ptr(tot), be.ptr(dj), be.ptr(dp), 69, be.ptr(db), 10,
                                        be.ptr(dc), n, be.stream), "body loss")
    k = "body%d" % int(ignore)
    errs = {}
    for name, got in (("parts", parts), ("reproj", reproj), ("djoints", dj), ("dpose", dp), ("dbetas", db), ("dcam_t", dc)):
        _within(name, be.host(got), g[f"{k}_{name}_f64"][sel], g[f"bound_{k}_{name}"], errs)
    _report("body loss %s ignore=%d" % (sel, ignore), errs)
    assert np.array_equal(be.host(tot), be.host(parts)[:, 4])
    assert np.array_equal(be.host(kp), kp_before)          # the mask is applied inside: the keypoints are read only
    if ignore:
        assert np.all(be.host(reproj)[:, [1, 9, 12, 27, 28]] == 0) and np.all(be.host(dj)[:, [1, 9, 12, 27, 28]] == 0)
    return errs


# ---------------------------------------------------------------------------------------- Adam
def case_adam(be, B=3, seed=5, lr=1e-2):
    """Three steps of group 1, a restart, three steps of group 2, against torch.optim.Adam on the CPU (a new optimiser per stage)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    pose, betas, cam = rn(B, 72) * 0.5, rn(B, 10) * 0.5, rn(B, 3) + torch.tensor([0.0, 0.0, 1.0])
    P, BE, CT = be.dev(pose.numpy()), be.dev(betas.numpy()), be.dev(cam.numpy())
    sb = be.lib.dyb_smplify_adam_state_bytes(B)
    state = be.dev(np.full(sb // 4, 7.0, np.float32))                   # stale moments and counts: the restart must not read them
    t_go, t_body, t_betas, t_cam = (t.clone().requires_grad_(True) for t in (pose[:, :3], pose[:, 3:], betas, cam))
    worst = 0.0
    for group, params in ((1, [t_go, t_cam]), (2, [t_body, t_betas, t_go])):
        opt = torch.optim.Adam(params, lr=lr, betas=(0.9, 0.999))
        for step in range(3):
            scale = 10.0 ** (step - 1)                                  # gradients of different sizes from step to step
            dpose, dbody_x, dbetas, dbetas_x, dcam = rn(B, 72) * scale, rn(B, 69) * scale, rn(B, 10) * scale, rn(B, 10), rn(B, 3) * scale
            before = [be.host(x).copy() for x in (P, BE, CT)]
            if group == 1:
                t_go.grad, t_cam.grad = dpose[:, :3].clone(), dcam.clone()
                rc = be.lib.dyb_smplify_adam(be.ptr(P), 72, be.ptr(BE), 10, be.ptr(CT), be.ptr(be.dev(dpose.numpy())), None, 0,
                                             be.ptr(be.dev(dbetas.numpy())), None, 0, be.ptr(be.dev(dcam.numpy())), be.ptr(state), sb, 1,
                                             int(step == 0), lr, 0.9, 0.999, 1e-8, B, be.stream)
            else:
                t_go.grad = dpose[:, :3].clone()
                t_body.grad, t_betas.grad = dpose[:, 3:] + dbody_x, dbetas + dbetas_x
                rc = be.lib.dyb_smplify_adam(be.ptr(P), 72, be.ptr(BE), 10, be.ptr(CT), be.ptr(be.dev(dpose.numpy())), be.ptr(be.dev(dbody_x.numpy())),
                                             69, be.ptr(be.dev(dbetas.numpy())), be.ptr(be.dev(dbetas_x.numpy())), 10, None, be.ptr(state), sb, 2,
                                             int(step == 0), lr, 0.9, 0.999, 1e-8, B, be.stream)
            _check(rc, "adam")
            opt.step()
            ref = [torch.cat([t_go, t_body], 1).detach().numpy(), t_betas.detach().numpy(), t_cam.detach().numpy()]
            got = [be.host(x) for x in (P, BE, CT)]
            e = max(float(np.abs(a - b).max()) for a, b in zip(got, ref))
            worst = max(worst, e)
            assert e < ADAM_TOL, (group, step, e)
            if group == 1:                          # the other group is left alone, bit for bit
                assert np.array_equal(got[0][:, 3:], before[0][:, 3:]) and np.array_equal(got[1], before[1])
            else:
                assert np.array_equal(got[2], before[2])
            st = be.host(state)
            m, v = st[:B * 85].reshape(B, 85), st[B * 85:2 * B * 85].reshape(B, 85)
            assert np.all(st[2 * B * 85:].view(np.int32) == step + 1)
            cols = {t_go: slice(0, 3), t_body: slice(3, 72), t_betas: slice(72, 82), t_cam: slice(82, 85)}
            for p in params:
                rm, rv = opt.state[p]["exp_avg"].numpy(), opt.state[p]["exp_avg_sq"].numpy()
                assert np.abs(m[:, cols[p]] - rm).max() <= ADAM_MOMENT_TOL * np.abs(rm).max(), (group, step, "m")
                assert np.abs(v[:, cols[p]] - rv).max() <= ADAM_MOMENT_TOL * np.abs(rv).max(), (group, step, "v")
    print("adam worst parameter deviation %.2e" % worst)
    return worst


# ---------------------------------------------------------------------------------------- the fit against goldens (b) / (c)
FIT_CLASSES = ("vertices", "joints", "pose", "betas", "cam_t", "reproj")


def check_fit(g, iters, sel, out, log, what):
    """out: dict of the six outputs (numpy) for the samples `sel`; log [2 * iters][len(sel)] or None."""
    errs = {}
    for n in FIT_CLASSES:
        ref = g[f"i{iters}_{n}_f64"][sel]
        got = out[n][:, g["vert_idx"]] if n == "vertices" else out[n]
        _within(n, got, ref, g["bound_" + n], errs)
    if iters:
        ref = g[f"i{iters}_loss_f64"][:, sel]
        log = np.asarray(log, np.float64)
        for it in range(2 * iters):                # per iteration, so that a wrong step is located
            stage = "cam" if it < iters else "body"
            e = float(np.abs(log[it] - ref[it]).max())
            errs.setdefault("loss_" + stage, (0.0, float(g["bound_loss_" + stage])))
            if e > errs["loss_" + stage][0]:
                errs["loss_" + stage] = (e, float(g["bound_loss_" + stage]))
            assert e <= float(g["bound_loss_" + stage]), (what, "loss of iteration", it, e, float(g["bound_loss_" + stage]))
    _report(what, errs)
    return errs


def run_fit_abi(be, g, tab, gmm, sel, iters, tables=None):
    sel, n = list(sel), len(sel)
    fb, ib, (_ka, pf), (_kb, pi) = tables if tables is not None else smpl_device_tables(be, tab)
    G = gmm_dev(be, gmm)
    D = lambda k: be.dev(g[k][sel])
    V, J, P, BE, CT, RP = be.empty((n, 6890, 3)), be.empty((n, 49, 3)), be.empty((n, 72)), be.empty((n, 10)), be.empty((n, 3)), be.empty((n, 49))
    LOG = be.empty((max(1, 2 * iters), n))
    wsb = be.lib.dyb_smplify_fit_workspace_bytes(n)
    ws = be.empty((wsb // 4,))
    kp = D("kp")
    kp_before = be.host(kp).copy()
    _check(be.lib.dyb_smplify_fit(pf, pi, be.ptr(G[0]), be.ptr(G[1]), be.ptr(G[2]), be.ptr(D("init_pose")), be.ptr(D("init_betas")),
                                  be.ptr(D("init_cam_t")), be.ptr(D("center")), be.ptr(kp), iters, 1e-2, 5000.0, be.ptr(V), be.ptr(J), be.ptr(P),
                                  be.ptr(BE), be.ptr(CT), be.ptr(RP), be.ptr(LOG) if iters else None, n, be.ptr(ws), wsb, be.stream), "fit")
    assert np.array_equal(be.host(kp), kp_before)
    out = dict(vertices=be.host(V), joints=be.host(J), pose=be.host(P), betas=be.host(BE), cam_t=be.host(CT), reproj=be.host(RP))
    return out, (be.host(LOG) if iters else None)


def case_fit(be, g, tab, gmm, sel, iters, tables=None):
    out, log = run_fit_abi(be, g, tab, gmm, sel, iters, tables)
    if iters == 0:                                  # the evaluation of the initial values: parameters come back as they went in
        for k, src in (("pose", "init_pose"), ("betas", "init_betas"), ("cam_t", "init_cam_t")):
            assert np.array_equal(out[k], g[src][list(sel)]), k
    return check_fit(g, iters, list(sel), out, log, "fit abi %s iters=%d" % (list(sel), iters)), out, log


# ---------------------------------------------------------------------------------------- margins of the golden
def check_margins(g):
    """The conditions tools/make_golden_smplify.py asserts, again from the stored data: the mixture component is the same at every
    iteration in fp32 and fp64 and its gap to the runner-up is >= 100 x the fp32-vs-fp64 difference of the two values; every optimised
    component's first-step gradient is >= 100 x its fp32-vs-fp64 difference."""
    worst = dict(gap=np.inf, grad=np.inf)
    for it in [int(i) for i in g["iters"] if int(i) > 0]:
        g32, g64 = g[f"i{it}_gmm_f32"], g[f"i{it}_gmm_f64"]
        assert np.array_equal(g32[..., 2], g64[..., 2]) and np.all(g64[..., 2] == g64[:1, :, 2]), it
        gap = g64[..., 1] - g64[..., 0]
        diff = np.maximum(np.abs(g32[..., 0] - g64[..., 0]), np.abs(g32[..., 1] - g64[..., 1]))
        worst["gap"] = min(worst["gap"], float((gap / np.maximum(diff, 1e-300)).min()))
        for tag in ("s1", "s2"):
            a, b = g[f"i{it}_g{tag}_f32"], g[f"i{it}_g{tag}_f64"]
            worst["grad"] = min(worst["grad"], float((np.abs(b) / np.maximum(np.abs(a - b), 1e-300)).min()))
    print("golden margins", worst)
    assert worst["gap"] >= MARGIN and worst["grad"] >= MARGIN, worst
    # the bounds are what the tool derived: 3 x the stored floors, nothing else
    for k in [k for k in g.files if k.startswith("floor_")]:
        assert float(g["bound_" + k[6:]]) == 3.0 * float(g[k])
    return worst


# ---------------------------------------------------------------------------------------- the Python surface (dynaboa_amd.smplify)
def make_fitter(tab, device, native, num_iters):
    from dynaboa_amd.smpl import SMPL
    from dynaboa_amd.smplify import SMPLify
    return SMPLify(step_size=1e-2, num_iters=num_iters, focal_length=5000, device=device, smpl=SMPL(tables=tab), native=native)


def call_fitter(fitter, g, sel, device):
    T = lambda k: torch.from_numpy(g[k][list(sel)]).to(device)
    kp = T("kp")
    kp_before = kp.clone()
    res = fitter(T("init_pose"), T("init_betas"), T("init_cam_t"), T("center"), kp)
    assert torch.equal(kp, kp_before), "the caller's keypoints_2d was written"       # (the reference zeroes five confidences in place)
    out = {n: r.detach().cpu().numpy() for n, r in zip(FIT_CLASSES, res)}
    log = None if fitter.last_losses is None else fitter.last_losses.detach().cpu().numpy()
    return out, log


def case_fitter(tab, g, device, native, iters, sel=(0, 1, 2)):
    """SMPLify.__call__ (native: dyb_smplify_fit; else the autograd composition) against goldens (b) / (c)."""
    out, log = call_fitter(make_fitter(tab, device, native, iters), g, sel, device)
    return check_fit(g, iters, list(sel), out, log, "SMPLify(native=%s) %s iters=%d" % (native, list(sel), iters)), out


def case_rodrigues_autograd(device, n=65):
    """smpl._rodrigues carries a gradient when its input requires one (it used to detach), with unchanged forward values."""
    from dynaboa_amd.smpl import _rodrigues
    aa, dR = rodrigues_inputs(n)
    x = torch.from_numpy(aa).to(device).requires_grad_(True)
    R = _rodrigues(x)
    assert torch.equal(R.detach(), _rodrigues(x.detach()))
    (gx,) = torch.autograd.grad((R * torch.from_numpy(dR).to(device)).sum(), x)
    x64 = torch.from_numpy(aa).double().requires_grad_(True)
    (ref,) = torch.autograd.grad((O.smplx_rodrigues(x64) * torch.from_numpy(dR).double()).sum(), x64)
    err = (gx.cpu().double() - ref).abs().max(1).values / ref.abs().max(1).values.clamp_min(1.0)
    assert float(err.max()) < RODRIGUES_TOL, float(err.max())


def case_refine(tab, g, device, native=True):
    """The crop bridge: input conversions against hand values; refine at num_iters = 0 followed by cam_t_to_crop_cam gives the camera back."""
    from dynaboa_amd import smplify as S
    cam = torch.tensor([[0.9, 0.02, -0.03], [1.1, -0.05, 0.04]], device=device)
    t = S.crop_cam_to_cam_t(cam)
    hand = np.array([[0.02, -0.03, 2 * 5000.0 / (224 * 0.9 + 1e-9)], [-0.05, 0.04, 2 * 5000.0 / (224 * 1.1 + 1e-9)]])
    assert np.abs(t.cpu().numpy() - hand).max() < 4e-6                       # (1 ulp of 49.6 is 3.8e-6)
    assert np.abs(S.cam_t_to_crop_cam(t).cpu().numpy() - cam.cpu().numpy()).max() < 2e-7
    kp = torch.tensor([[[-1.0, 1.0, 0.5], [0.0, 0.25, 1.0]]], device=device)
    assert np.array_equal(S.crop_kp_to_pixels(kp).cpu().numpy(), np.array([[[0.0, 224.0, 0.5], [112.0, 140.0, 1.0]]], np.float32))
    fitter = make_fitter(tab, device, native, 0)
    sel = [0, 2]
    rot = O.smplx_rodrigues(torch.from_numpy(g["init_pose"][sel]).reshape(-1, 3)).view(2, 24, 3, 3).to(device)
    betas = torch.from_numpy(g["init_betas"][sel]).to(device)
    kpn = torch.from_numpy(g["kp"][sel]).to(device)
    kpn = torch.cat([(kpn[..., :2] - 112.0) / 112.0, kpn[..., 2:]], -1)
    r = fitter.refine(rot, betas, cam, kpn)
    assert set(r) >= {"vts", "rotmat", "shape", "cam", "pose", "cam_t", "reprojection_loss"}
    assert np.abs(r["cam"].cpu().numpy() - cam.cpu().numpy()).max() < 2e-7            # an unmoved camera comes back
    assert torch.equal(r["shape"], betas)
    # rotation -> axis-angle -> rotation: the pose is the same rotation (the conversion's fp32 accuracy, as kernel_cases.case_rotmat_to_aa)
    assert float((r["rotmat"].cpu() - rot.cpu()).abs().max()) < 1e-5
    assert r["vts"].shape == (2, 6890, 3) and r["reprojection_loss"].shape == (2, 49)
    # the same call through __call__ with hand-converted inputs gives the same bytes
    out = fitter(r["pose"], betas, t, torch.full((2, 2), 112.0, device=device), S.crop_kp_to_pixels(kpn))
    assert torch.equal(out[5], r["reprojection_loss"]) and torch.equal(out[0], r["vts"])


def case_get_fitting_loss(tab, g, device, sel=(1, 2)):
    """get_fitting_loss on a fit's outputs is that fit's final evaluation (same kernels, same inputs: the same bytes)."""
    f = make_fitter(tab, device, True, 1)
    T = lambda k: torch.from_numpy(g[k][list(sel)]).to(device)
    kp = T("kp")
    kp0 = kp.clone()
    _v, _j, pose, betas, cam_t, reproj = f(T("init_pose"), T("init_betas"), T("init_cam_t"), T("center"), kp)
    again = f.get_fitting_loss(pose, betas, cam_t, T("center"), kp)
    assert torch.equal(kp, kp0)
    assert torch.equal(again, reproj)
