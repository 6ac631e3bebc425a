"""Kernel-level cases of the keypoint-set window (dyb_frame_losses_kp, dyb_aux_loss_terms_kp: csrc/losses.hip), shared by
tests/test_online_emu.py (host build of the kernels) and tests/test_online_gpu.py (MI355X).  References: torch-CPU autograd of the
reference's own formulas (tests/online_ref.py).  Tolerances are the ones kernel_cases.case_frame_losses (5e-4) and case_aux_terms (2e-4)
use against the same kind of reference; shapes are the smallest that reach every path: B = 1, and B = 2 / 3 for the per-sample strides
and the batch means."""
import numpy as np
import torch

import online_ref as R
from conftest import rel_err
from oracle import ref_cpu as O

FRAME_TOL = 5e-4
AUX_TOL = 2e-4
W2D, WSHAPE, WPOSE = 10.0, 2e-6, 1e-4


def _frame_inputs(B, seed, conf="rand"):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    rot = O.smplx_rodrigues(rn(B * 24, 3) * 0.3).view(B, 24, 3, 3)
    shape = rn(B, 10) * 0.5
    cam = torch.tensor([0.9, 0.02, -0.03]) + 0.05 * rn(B, 3)
    joints = rn(B, 49, 3) * 0.3
    kp = torch.cat([torch.rand(B, 49, 2, generator=g) * 2 - 1, (torch.rand(B, 49, 1, generator=g) < 0.8).float()], -1)
    if conf == "slot24":            # the one joint the gt24-sized staging arrays had no room for
        kp[:, :, 2] = 0.0
        kp[:, 24, 2] = 1.0
    elif conf == "gt_only":         # confident ground-truth style slots only: nothing of it may reach an op25 result
        kp[:, :25, 2] = 0.0
        kp[:, 25:, 2] = 1.0
    return dict(rot=rot, shape=shape, cam=cam, joints=joints, kp=kp)


def _gmm_dev(be, gmm):
    logw = np.log(gmm["nll_weights"]).astype(np.float32).reshape(-1)
    return be.dev(gmm["means"]), be.dev(gmm["precisions"]), be.dev(logw)


def _run_frame(be, x, G, kp_set, B, export="kp"):
    D = lambda t: be.dev(t.detach().numpy() if torch.is_tensor(t) else t)
    L = be.empty((4,))
    DR, DS, DC, DJ = be.empty((B, 24, 9)), be.empty((B, 10)), be.empty((B, 3)), be.empty((B, 49, 3))
    ws = be.empty((B * 4,))
    head = (be.ptr(D(x["rot"])), be.ptr(D(x["shape"])), 10, be.ptr(D(x["cam"])), 3, be.ptr(D(x["joints"])), be.ptr(D(x["kp"])),
            be.ptr(G[0]), be.ptr(G[1]), be.ptr(G[2]), W2D, WSHAPE, WPOSE, be.ptr(L), be.ptr(DR), be.ptr(DS), 10, be.ptr(DC), 3, be.ptr(DJ), B)
    if export == "kp":
        rc = be.lib.dyb_frame_losses_kp(*head, kp_set, be.ptr(ws), B * 16, be.stream)
    else:
        rc = be.lib.dyb_frame_losses(*head, be.ptr(ws), B * 16, be.stream)
    return rc, [be.host(a).copy() for a in (L, DR, DS, DC, DJ)]


def case_frame_op25(be, gmm, B, seed=11, conf="rand"):
    """Frame head with the op25 window: the four loss values and the four gradients against torch autograd of dynaboa_webcam.py:256-261."""
    x = _frame_inputs(B, seed, conf)
    gm = {k: torch.from_numpy(v) for k, v in gmm.items()}
    t = {k: x[k].clone().requires_grad_(True) for k in ("rot", "shape", "cam", "joints")}
    l2d, lsh, lpo, tot = R.frame_total(t["rot"], t["shape"], t["cam"], t["joints"], x["kp"], gm, "op25", W2D, WSHAPE, WPOSE)
    gr, gs, gc, gj = torch.autograd.grad(tot, [t["rot"], t["shape"], t["cam"], t["joints"]], allow_unused=True)
    gc = torch.zeros(B, 3) if gc is None else gc
    gj = torch.zeros(B, 49, 3) if gj is None else gj
    rc, (Lh, DR, DS, DC, DJ) = _run_frame(be, x, _gmm_dev(be, gmm), R.KP_CODE["op25"], B)
    assert rc == 0, rc
    rel = lambda a, b: abs(float(a) - float(b)) / abs(float(b)) if float(b) != 0 else abs(float(a))
    e = dict(l2d=rel(Lh[0], l2d), lsh=rel(Lh[1], lsh), lpo=rel(Lh[2], lpo), total=rel(Lh[3], tot),
             drot=rel_err(DR.reshape(B, 24, 3, 3), gr.numpy()), dshape=rel_err(DS, gs.numpy()),
             dcam=rel_err(DC, gc.numpy()) if float(gc.abs().max()) > 0 else float(np.abs(DC).max()),
             djoints=rel_err(DJ, gj.numpy()) if float(gj.abs().max()) > 0 else float(np.abs(DJ).max()))
    print("frame op25", B, conf, e)
    assert max(e.values()) < FRAME_TOL, e
    if conf == "slot24":
        # joint 24 alone carries the term: correct (above), non-zero, and nothing leaks into another row
        assert Lh[0] > 0 and np.abs(DJ[:, 24]).min() > 0 and np.abs(DC).max() > 0
        rest = np.delete(DJ, 24, axis=1)
        assert np.all(rest == 0.0), np.abs(rest).max()
    if conf == "gt_only":
        # confident slots 25..48 are outside the op25 window: the 2-D term is exactly 0 and dcam has no other source
        assert Lh[0] == 0.0 and np.all(DC == 0.0) and np.all(DJ == 0.0)
        assert rel(Lh[3], WSHAPE * float(Lh[1]) + WPOSE * float(Lh[2])) < 1e-6
    return e


def case_frame_gt24_bit_identical(be, golden, gmm):
    """gt24 through the new export against dyb_frame_losses on golden g4's inputs: every output equal bit for bit."""
    g = golden("g4_losses.npz")
    B = g["shape"].shape[0]
    x = dict(rot=O.smplx_rodrigues(torch.from_numpy(g["aa"])).view(B, 24, 3, 3), shape=g["shape"], cam=g["cam"], joints=g["s3d"], kp=g["kp"])
    G = _gmm_dev(be, gmm)
    rc0, old = _run_frame(be, x, G, 0, B, export="plain")
    rc1, new = _run_frame(be, x, G, R.KP_CODE["gt24"], B)
    assert rc0 == 0 and rc1 == 0
    for name, a, b in zip(("losses", "drot", "dshape", "dcam", "djoints"), old, new):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
    assert abs(old[0][0] - g["l2d"]) / abs(g["l2d"]) < FRAME_TOL          # (and it is still the golden's value)


def _motion_inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    cam_of = lambda: torch.tensor([0.9, 0.02, -0.03]) + 0.05 * rn(B, 3)
    kp_of = lambda: torch.cat([torch.rand(B, 49, 2, generator=g) * 2 - 1, (torch.rand(B, 49, 1, generator=g) < 0.7).float()], -1)
    x = dict(rot=torch.eye(3).expand(B, 24, 3, 3) + 0.3 * rn(B, 24, 3, 3), shape=rn(B, 10) * 0.5, cam=cam_of(), joints=rn(B, 49, 3) * 0.3,
             cam2=cam_of(), joints2=rn(B, 49, 3) * 0.3, kp=kp_of(), kp2=kp_of())
    # the mask: joint 3 confident in this frame only, joint 5 in the history frame only, joint 7 in both, joint 30 (outside the
    # window) in both
    x["kp"][0, 3, 2], x["kp2"][0, 3, 2] = 1.0, 0.0
    x["kp"][0, 5, 2], x["kp2"][0, 5, 2] = 0.0, 1.0
    x["kp"][0, 7, 2], x["kp2"][0, 7, 2] = 1.0, 1.0
    x["kp"][0, 30, 2], x["kp2"][0, 30, 2] = 1.0, 1.0
    return x


def _run_motion(be, x, B, acc, w, kp_set, pre=0.25):
    D = lambda t: be.dev(t.detach().numpy())
    vals = be.dev(np.full(5, pre, np.float32))
    d_rot, d_shape, d_cam, d_j = (be.dev(np.full(s, pre, np.float32)) for s in ((B, 216), (B, 10), (B, 3), (B, 147)))
    d_cam2, d_j2 = be.dev(np.full((B, 3), pre, np.float32)), be.dev(np.full((B, 147), pre, np.float32))
    rc = be.lib.dyb_aux_loss_terms_kp(1, B, acc, w, be.ptr(D(x["rot"])), be.ptr(D(x["shape"])), 10, be.ptr(D(x["cam"])), 3, be.ptr(D(x["joints"])),
                                      None, None, 0, be.ptr(D(x["cam2"])), 3, be.ptr(D(x["joints2"])), be.ptr(D(x["kp"])), be.ptr(D(x["kp2"])),
                                      None, None, None, be.ptr(vals), be.ptr(d_rot), be.ptr(d_shape), be.ptr(d_cam), be.ptr(d_j), be.ptr(d_cam2),
                                      be.ptr(d_j2), kp_set, be.stream)
    return rc, [be.host(a).copy() for a in (vals, d_rot, d_shape, d_cam, d_j, d_cam2, d_j2)]


def case_motion_op25(be, B, seed=17):
    """Motion term with the op25 window: value and gradients to the student and the history pass against torch autograd of
    dynaboa_webcam.py:164-182, accumulate 0 and 1."""
    x = _motion_inputs(B, seed)
    w, pre = 0.8, np.float32(0.25)
    t = {k: x[k].clone().requires_grad_(True) for k in ("cam", "joints", "cam2", "joints2")}
    loss = R.motion_loss(t["cam"], t["joints"], t["cam2"], t["joints2"], x["kp"], x["kp2"], "op25")
    gc, gj, gc2, gj2 = torch.autograd.grad(loss * w, [t["cam"], t["joints"], t["cam2"], t["joints2"]])
    assert float(loss) > 0 and float(gj[0, 7].abs().max()) > 0
    assert float(gj[0, 3].abs().max()) == 0 and float(gj[0, 5].abs().max()) == 0 and float(gj[:, 25:].abs().max()) == 0     # the mask, the window
    out = {}
    for acc in (0, 1):
        rc, o = _run_motion(be, x, B, acc, w, R.KP_CODE["op25"], pre)
        assert rc == 0, rc
        out[acc] = o
    v = out[0][0]
    e = dict(val=abs(float(v[0]) - float(loss)) / float(loss), total=abs(float(v[4]) - float(loss)) / float(loss),
             d_cam=rel_err(out[0][3], gc.numpy()), d_joints=rel_err(out[0][4], gj.reshape(B, 147).numpy()),
             d_cam2=rel_err(out[0][5], gc2.numpy()), d_joints2=rel_err(out[0][6], gj2.reshape(B, 147).numpy()),
             # accumulate = 1 adds to what is there (0.25 + g rounds at 3e-8: the denominator of kernel_cases.case_aux_terms)
             d_cam_acc=float(np.abs(out[1][3] - pre - gc.numpy()).max() / (np.abs(gc.numpy()).max() + 1e-3)),
             d_joints_acc=float(np.abs(out[1][4] - pre - gj.reshape(B, 147).numpy()).max() / (np.abs(gj.numpy()).max() + 1e-3)))
    print("motion op25", B, e)
    assert max(e.values()) < AUX_TOL, e
    assert np.all(v[1:4] == 0)
    # the motion term has no rotation / shape gradient: written as zero, left alone when accumulating
    assert np.all(out[0][1] == 0) and np.all(out[0][2] == 0) and np.all(out[1][1] == pre) and np.all(out[1][2] == pre)
    # joints outside the window and joints the mask drops receive exactly nothing in either pass
    for arr in (out[0][4], out[0][6]):
        a = arr.reshape(B, 49, 3)
        assert np.all(a[:, 25:] == 0) and np.all(a[0, 3] == 0) and np.all(a[0, 5] == 0) and np.abs(a[0, 7]).max() > 0
    return e


def case_replicas(be, gmm, B=2):
    """Two replicas with different inputs in ONE launch of each windowed head: each replica's outputs equal its launch alone bit for bit."""
    G = _gmm_dev(be, gmm)
    xs = [_frame_inputs(B, 31), _frame_inputs(B, 32)]
    nin, nout = B * (216 + 10 + 3 + 147 + 147), 4 + B * (216 + 10 + 3 + 147 + 4)
    per = (nin + nout + 63) // 64 * 64
    blob = np.full((2, per), np.nan, np.float32)
    for r, x in enumerate(xs):
        blob[r, :nin] = np.concatenate([x[k].numpy().ravel() for k in ("rot", "shape", "cam", "joints", "kp")])
    Bd = be.dev(blob)
    rc = be.lib.dyb_debug_frame_losses_kp_replicas(be.ptr(Bd), per, 2, be.ptr(G[0]), be.ptr(G[1]), be.ptr(G[2]), W2D, WSHAPE, WPOSE, B,
                                                   R.KP_CODE["op25"], be.stream)
    assert rc == 0, rc
    got = be.host(Bd)
    for r, x in enumerate(xs):
        rc, alone = _run_frame(be, x, G, R.KP_CODE["op25"], B)
        assert rc == 0
        o = nin
        for name, a in zip(("losses", "drot", "dshape", "dcam", "djoints"), alone):
            seg = got[r, o:o + a.size]
            assert np.array_equal(seg.view(np.uint32), a.ravel().view(np.uint32)), (r, name)
            o += a.size
    assert not np.array_equal(got[0, nin:nin + 4], got[1, nin:nin + 4])          # (the replicas did see different inputs)
    # motion term
    ms = [_motion_inputs(B, 41), _motion_inputs(B, 42)]
    keys = ("rot", "shape", "cam", "joints", "cam2", "joints2", "kp", "kp2")
    nin = B * (216 + 10 + 3 + 147 + 3 + 147 + 147 + 147)
    nout = 8 + B * (216 + 10 + 3 + 147 + 3 + 147)
    per = (nin + nout + 63) // 64 * 64
    blob = np.full((2, per), np.nan, np.float32)
    for r, x in enumerate(ms):
        blob[r, :nin] = np.concatenate([x[k].numpy().ravel() for k in keys])
    Bd = be.dev(blob)
    rc = be.lib.dyb_debug_motion_term_kp_replicas(be.ptr(Bd), per, 2, B, 0, 0.8, R.KP_CODE["op25"], be.stream)
    assert rc == 0, rc
    got = be.host(Bd)
    for r, x in enumerate(ms):
        rc, alone = _run_motion(be, x, B, 0, 0.8, R.KP_CODE["op25"])
        assert rc == 0
        assert np.array_equal(got[r, nin:nin + 5].view(np.uint32), alone[0].view(np.uint32)), (r, "vals")
        o = nin + 8
        for name, a in zip(("d_rot", "d_shape", "d_cam", "d_joints", "d_cam2", "d_joints2"), alone[1:]):
            seg = got[r, o:o + a.size]
            assert np.array_equal(seg.view(np.uint32), a.ravel().view(np.uint32)), (r, name)
            o += a.size
    assert got[0, nin] != got[1, nin]


def case_unknown_set(be, gmm, B=1):
    """An unknown keypoint set is DYB_ERR_ARG (-1) from both exports and nothing is written."""
    G = _gmm_dev(be, gmm)
    x = _frame_inputs(B, 5)
    for bad in (2, -1, 25):
        rc, outs = _run_frame(be, x, G, bad, B)
        assert rc == -1, (bad, rc)
        assert all(np.all(np.isnan(a)) for a in outs), bad            # (the output buffers were NaN-filled)
        m = _motion_inputs(B, 6)
        for mode_kp in (bad,):
            rc, outs = _run_motion(be, m, B, 0, 0.8, mode_kp, pre=0.25)
            assert rc == -1, (bad, rc)
            assert all(np.all(a == np.float32(0.25)) for a in outs), bad
    # the set is checked for the modes that do not read it, too (teacher: mode 0)
    D = lambda t: be.dev(t.numpy())
    m = _motion_inputs(B, 7)
    vals, d_rot, d_shape, d_cam, d_j = be.empty((5,)), be.empty((B, 216)), be.empty((B, 10)), be.empty((B, 3)), be.empty((B, 147))
    args = (0, B, 0, 0.1, be.ptr(D(m["rot"])), be.ptr(D(m["shape"])), 10, be.ptr(D(m["cam"])), 3, be.ptr(D(m["joints"])), be.ptr(D(m["rot"])),
            be.ptr(D(m["shape"])), 10, be.ptr(D(m["cam2"])), 3, be.ptr(D(m["joints2"])), None, None, None, None, None, be.ptr(vals), be.ptr(d_rot),
            be.ptr(d_shape), be.ptr(d_cam), be.ptr(d_j), None, None)
    assert be.lib.dyb_aux_loss_terms_kp(*args, 7, be.stream) == -1 and np.all(np.isnan(be.host(vals)))
    v = {}
    for s in (0, 1):                                                  # modes 0 and 2 do not depend on the set
        assert be.lib.dyb_aux_loss_terms_kp(*args, s, be.stream) == 0
        v[s] = (be.host(vals).copy(), be.host(d_j).copy())
    assert np.array_equal(v[0][0], v[1][0]) and np.array_equal(v[0][1], v[1][1])


# ---------------------------------------------------------------------------------------- streams (goldens g9_online_*)
STREAM_OPTS = {
    "boa_i2": dict(use_boa=1, interval=2, dynamic_boa=0),
    "boa_i2_gated": dict(use_boa=1, interval=2, dynamic_boa=1, optim_steps=2),
    "plain": dict(use_boa=0),
}
SLICE_PARAMS = ["conv1.weight", "layer1.0.conv2.weight", "layer2.0.conv2.weight", "layer3.5.conv1.weight", "layer4.0.conv2.weight",
                "layer4.2.bn3.weight", "fc1.weight", "fc2.weight", "decpose.weight", "decpose.bias", "deccam.bias"]


def online_noise_bounds(tag, names):
    """Bounds from tests/golden/g9_online_<tag>_noise.npz (tools/make_golden_online.py: the reference in fp32 with and without oneDNN,
    each against the reference's own code in double on the same stream), by conftest.noise_bounds' rule: a tensor's bound is
    NOISE_FACTOR x the largest deviation either fp32 draw shows over the tensor's class (stage x kind), never below NOISE_MIN (slice
    cosines of Adam-normalised quantities: ADAM_SLICE_FLIP).  -> {q: dict(nd [169], cos [169], frame_nd [nframes][169])}."""
    from conftest import ADAM_SLICE_FLIP, NOISE_FACTOR, NOISE_MIN, golden, tensor_class
    z = golden(f"g9_online_{tag}_noise.npz")
    assert [str(x) for x in z["names"]] == list(names)
    cls = [tensor_class(n) for n in names]

    def pooled(x):                               # [..., 169] -> the class maximum at every tensor's place
        x = np.asarray(x, np.float64)
        out = np.empty_like(x)
        for c in set(cls):
            idx = [i for i, ci in enumerate(cls) if ci == c]
            out[..., idx] = x[..., idx].max(axis=-1, keepdims=True)
        return out
    res = {}
    for q in ("m", "v", "d", "t"):
        if f"{q}_nd_ref" not in z.files:
            continue
        draws = [d for d in ("ref", "o2") if f"{q}_nd_{d}" in z.files]
        nd = np.max([z[f"{q}_nd_{d}"] for d in draws], axis=0)
        cs = 1.0 - np.min([z[f"{q}_cos_{d}"] for d in draws], axis=0)
        fnd = np.max([z[f"frame_{q}_nd_{d}"] for d in draws], axis=0)
        cmin = ADAM_SLICE_FLIP if q in ("d", "t") else NOISE_MIN["cos"]
        res[q] = dict(nd=np.maximum(NOISE_MIN["nd"], NOISE_FACTOR * pooled(nd)), cos=1.0 - np.maximum(cmin, NOISE_FACTOR * pooled(cs)),
                      frame_nd=np.maximum(NOISE_MIN["nd"], NOISE_FACTOR * pooled(fnd)))
    return res


class OnlineStream:
    """One golden stream through OnlineAdaptor: mode 'autograd' (native_step 0), 'native' (the stepper), 'replica' (replica 0 of a
    2-replica OnlineGroup whose replica 1 sees other frames).  check_frame / check_end hold the run against the golden."""

    def __init__(self, tag, mode, device="cuda:0", log_frames=8):
        from conftest import golden
        from dynaboa_amd import online as ON
        from dynaboa_amd.base_adaptor import synthetic_bundle
        self.tag, self.mode, self.g = tag, mode, golden(f"g9_online_{tag}.npz")
        g = self.g
        opts = dict(STREAM_OPTS[tag])
        if "gate_threshold" in g.files:
            opts["cos_sim_threshold"] = float(g["gate_threshold"])
        self.opts = opts
        self.K = int(opts.get("optim_steps", 7)) if opts.get("dynamic_boa") else 0
        self.seed = int(g["frame_seed"]) if "frame_seed" in g.files else 22
        mk = lambda: ON.OnlineAdaptor(ON.online_options(**opts, native_step=0 if mode == "autograd" else 1, log_frames=log_frames),
                                      synthetic_bundle(seed=22, identity_pose=False, randomize_norm=True, smpl_seed=0), device=device)
        self.ad = mk()
        self.group = ON.OnlineGroup([self.ad, mk()]) if mode == "replica" else None
        self.hmr = getattr(self.ad.model, "module", self.ad.model)
        self.theta0 = self.hmr.theta.detach().clone()
        self.names = [str(x) for x in g["names"]]
        self.nb = online_noise_bounds(tag, self.names)
        self.n = 0

    def frame(self):
        from dynaboa_amd import assets
        ad, n = self.ad, self.n
        dev = ad.device
        fr = {k: v.to(dev) for k, v in assets.make_online_frame(n, seed=self.seed).items()}
        if self.group is not None:
            other = {k: v.to(dev) for k, v in assets.make_online_frame(n + 100, seed=self.seed).items()}
            res = self.group.step_processed([(fr["image"], fr["smpl_j2d"], None), (other["image"], other["smpl_j2d"], None)])[0]
        else:
            res = ad.adapt_processed(fr["image"], fr["smpl_j2d"])
        if self.mode != "autograd" and ad.options.use_boa:
            assert ad._native is not None, ad._native_why
        self.check_frame(res)
        self.n += 1
        return res

    def state(self):
        ad, hmr = self.ad, self.hmr
        st = ad.optimizer.state[hmr.theta]
        L = hmr._layout1
        out = dict(m=L.unpack(st["exp_avg"]), v=L.unpack(st["exp_avg_sq"]),
                   d=L.unpack((hmr.theta.detach().double() - self.theta0.double()).float()))
        if "t" in self.nb:
            out["t"] = L.unpack((ad.teacher.theta.detach().double() - self.theta0.double()).float())
        return int(st["step"]), out

    def check_frame(self, res):
        from conftest import cosine
        ad, g, n, K = self.ad, self.g, self.n, self.K
        log = {k: float(v) for k, v in ad.fit_losses.items()}
        extra = int(g["extra_steps"][n])
        up = g["upper_terms"][n, min(extra, K)]              # the last upper level that ran: s2d, shape, pose, motion, teacher, total
        tot = abs(float(up[5]))
        o = ad.options
        w = dict(s2d=o.s2dloss_weight, shape=o.shape_prior_weight, pose=o.pose_prior_weight, motion=o.motionloss_weight, teacher=o.teacherloss_weight)
        if o.use_boa:
            ours_low = [log["ll/s2dloss"], log["ll/shape_prior"], log["ll/pose_prior"], log["ll/total"]]
            ours_up = dict(s2d=log["ul/s2dloss"], shape=log["ul/shape_prior"], pose=log["ul/pose_prior"], motion=log.get("ul/motion_loss"),
                           teacher=log.get("teacher/loss"), total=log["ul/total"])
            low = g["lower_terms"][n]
            assert abs(ours_low[3] - low[3]) < 1e-4 * abs(low[3]), (n, "lower total", ours_low[3], low[3])
            for k, a, b in zip(("s2d", "shape", "pose"), ours_low, low):
                assert w[k] * abs(a - b) < 1e-4 * abs(low[3]), (n, "lower", k, a, b)
                assert abs(a - b) < 1e-3 * abs(b), (n, "lower", k, a, b)
        else:
            ours_up = dict(s2d=log["ll/s2dloss"], shape=log["ll/shape_prior"], pose=log["ll/pose_prior"], motion=None, teacher=None, total=log["ll/total"])
        # the total to the 1e-4 the g5 streams hold theirs to; every term to the same ABSOLUTE accuracy in its weighted contribution
        # (a term is a summand of the total) AND relative to itself - the weights 2e-6 / 1e-4 would otherwise leave the priors
        # unconstrained: s2d, shape prior and pose prior to 1e-3 (smooth functions of the prediction, which is held to 1e-3 below), the two
        # small difference terms to 1 % of themselves (differences of two nearby predictions; what the gate values are held to)
        assert abs(ours_up["total"] - up[5]) < 1e-4 * tot, (n, "upper total", ours_up["total"], up[5])
        for i, k in enumerate(("s2d", "shape", "pose", "motion", "teacher")):
            if np.isnan(up[i]):
                assert ours_up[k] is None or (k == "motion" and ours_up[k] == 0.0), (n, k, "a term the reference did not evaluate")
                continue
            assert ours_up[k] is not None, (n, k)
            assert w[k] * abs(ours_up[k] - up[i]) < 1e-4 * tot, (n, k, ours_up[k], up[i])
            assert abs(ours_up[k] - up[i]) < (1e-2 if k in ("motion", "teacher") else 1e-3) * abs(up[i]), (n, k, ours_up[k], up[i])
        assert ad.last_extra_steps == extra, (n, ad.last_extra_steps, extra)
        if K:
            thr = float(g["gate_threshold"])
            sims = ad.feat_sims[ad.global_step]
            nchk = int(g["gate_checks"][n])
            assert len(sims) == nchk, (n, len(sims), nchk)
            for k in range(nchk):
                ours, refd = float(sims[k][12]["cos"]), float(g["gate_1mcos12"][n, k])
                dev = abs((1.0 - ours) - refd)
                assert ((1.0 - ours) > thr) == (refd > thr), (n, k)
                assert dev < 0.5 * abs(refd - thr) and dev < 1e-2 * refd, (n, k, 1.0 - ours, refd, thr)
                assert abs(ours - float(g["gate_cos12_64"][n, k])) < 3e-6, (n, k)
        for k, v in dict(rotmat=res["rotmat"], shape=res["shape"], cam=res["cam"]).items():
            assert rel_err(v.detach().cpu().numpy().reshape(g[f"pred{n}_{k}"].shape), g[f"pred{n}_{k}"]) < 1e-3, (n, k)
        vts = res["vts"].detach().double()
        vs = np.array([float(vts.sum()), float(vts.abs().sum())])
        assert abs(vs[1] - g[f"pred{n}_vsum"][1]) < 1e-3 * g[f"pred{n}_vsum"][1], (n, "vertices")
        step, st = self.state()
        assert step == int((g["step_frame"] <= n).sum()), (n, step)
        for q, key in (("m", "frame_m_norms"), ("v", "frame_v_norms"), ("d", "frame_delta_norms"), ("t", "frame_teacher_delta_norms")):
            if q not in self.nb or q not in st:
                continue
            x = np.array([float(st[q][k].double().norm()) for k in self.names])
            ref = g[key][n]
            e = np.abs(x - ref) / np.where(ref > 0, ref, 1.0)
            b = self.nb[q]["frame_nd"][n]
            bad = [(self.names[j], float(e[j]), float(b[j])) for j in range(len(e)) if e[j] >= b[j]]
            assert not bad, (self.tag, n, q, "norm deviation beyond 3 x the class floor", bad[:6])
        if n == 0 and extra == 0:
            # frame 0: after the first Adam step m = (1 - beta1) g - the outer gradient itself, at the existing frame-0 check's bounds
            g1 = self.hmr._layout1.unpack(ad.optimizer.state[self.hmr.theta]["exp_avg"] / (1 - o.beta1))
            gn = np.array([float(g1[k].double().norm()) for k in self.names])
            err = np.abs(gn - g["g1_norms"]) / g["g1_norms"]
            sl = {k: cosine(g1[k].flatten()[:256].double().cpu().numpy(), g["gstep_" + k][0]) for k in SLICE_PARAMS}
            print("frame-0 outer gradient: norm error median %.2e max %.2e; worst slice cosine %.6f" % (np.median(err), err.max(), min(sl.values())))
            assert np.median(err) < 1e-3 and err.max() < 1e-2, (float(np.median(err)), float(err.max()))
            assert min(sl.values()) >= 0.9999, sl

    def check_end(self):
        from conftest import cosine
        g = self.g
        step, st = self.state()
        assert step == int(g["adam_steps"])
        for k in [k[2:] for k in g.files if k.startswith("m_") and k != "m_norms"]:
            j = self.names.index(k)
            for q in ("m", "d"):
                c = cosine(st[q][k].flatten()[:256].double().cpu().numpy(), g[f"{q}_{k}"])
                assert c > self.nb[q]["cos"][j], (self.tag, q, k, c, float(self.nb[q]["cos"][j]))


def run_online_stream(tag, mode, log_frames=8):
    s = OnlineStream(tag, mode, log_frames=log_frames)
    for _ in range(int(s.g["nframes"])):
        s.frame()
    s.check_end()
    return s
