"""The online path end to end on the MI355X: the reference's ``dynaboa_webcam.py::Adaptor.online_adaptation`` streams (goldens
g9_online_*, tools/make_golden_online.py) through ``dynaboa_amd.online.OnlineAdaptor`` - on the autograd composition, on the native
stepper and as one replica of a group -, reload(), and the driver."""
import os

import numpy as np
import pytest
import torch

import online_cases as C

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BOA = ["boa_i2", "boa_i2_gated"]


@pytest.mark.parametrize("tag", BOA + ["plain"])
def test_stream_on_the_autograd_composition(tag):
    C.run_online_stream(tag, "autograd")


@pytest.mark.parametrize("tag", BOA)
def test_stream_on_the_native_stepper(tag):
    s = C.run_online_stream(tag, "native")
    assert s.ad._native is not None and s.ad._native.full


@pytest.mark.parametrize("tag", BOA)
def test_stream_as_replica_0_of_a_group(tag):
    C.run_online_stream(tag, "replica")


@pytest.mark.parametrize("mode", ["native", "replica"])
def test_stream_with_a_log_ring_shorter_than_the_stream(mode):
    """log_frames 2 on the 5-frame stream: the stepper's loss log wraps twice, every frame still reads its own slot."""
    s = C.run_online_stream("boa_i2", mode, log_frames=2)
    assert s.ad._native.frame <= 2 and s.ad.global_step == 5


def test_gated_stream_exercises_both_exits():
    from conftest import golden                                   # (the golden alone: what the gated runs above are held to)
    z = golden("g9_online_boa_i2_gated.npz")
    steps, K = z["extra_steps"].tolist(), 2
    assert any(1 <= e <= K for e in steps) and any(e == K + 1 for e in steps) and float(z["gate_margin"]) >= 0.02


@pytest.mark.parametrize("tag", BOA)
def test_native_stepper_agrees_with_the_autograd_composition(tag):
    """The agreement test_adaptation_gpu.test_native_full_term_set_matches_autograd_path asserts for the full term set: weights and
    teacher to 5e-6, Adam moments to 5e-3 (the ReLU-flip noise class)."""
    runs = []
    for mode in ("native", "autograd"):
        s = C.OnlineStream(tag, mode)
        for _ in range(int(s.g["nframes"])):
            s.frame()
        st = s.ad.optimizer.state[s.hmr.theta]
        runs.append(dict(theta=s.hmr.theta.detach().clone(), teacher=s.ad.teacher.theta.detach().clone(), m=st["exp_avg"].clone(),
                         v=st["exp_avg_sq"].clone(), step=int(st["step"])))
    a, b = runs
    rel = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm())
    assert a["step"] == b["step"]
    assert rel(a["theta"], b["theta"]) < 5e-6 and rel(a["teacher"], b["teacher"]) < 5e-6
    assert rel(a["m"], b["m"]) < 5e-3 and rel(a["v"], b["v"]) < 5e-3


def test_reload_restores_checkpoint_teacher_and_adam_and_the_stepper_follows():
    outs = []
    for mode in ("native", "autograd"):
        s = C.OnlineStream("boa_i2", mode)
        t_teacher0 = s.ad.teacher.theta.detach().clone()
        for _ in range(2):
            s.frame()
        ad = s.ad
        assert float((s.hmr.theta.detach() - s.theta0).abs().max()) > 0
        hist, gs = dict(ad.history), ad.global_step
        ad.reload()
        st = ad.optimizer.state[s.hmr.theta]
        assert torch.equal(s.hmr.theta.detach(), s.theta0) and torch.equal(ad.teacher.theta.detach(), t_teacher0)
        assert int(st["step"]) == 0 and float(st["exp_avg"].abs().max()) == 0 and float(st["exp_avg_sq"].abs().max()) == 0
        assert ad.global_step == gs and ad.history.keys() == hist.keys()              # history and the step counter stay
        if mode == "native":
            assert int(ad._native.lib.dyb_stepper_get_i(ad._native.h, b"adam_step")) == 0
        from dynaboa_amd import assets
        fr = {k: v.to(ad.device) for k, v in assets.make_online_frame(2, seed=22).items()}
        ad.adapt_processed(fr["image"], fr["smpl_j2d"])
        assert int(ad.optimizer.state[s.hmr.theta]["step"]) == 1
        assert "ul/motion_loss" in ad.fit_losses                                       # the history survived: frame 2 has its motion term
        outs.append((s.hmr.theta.detach().clone(), st["exp_avg"].clone()))
    rel = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm())
    assert rel(outs[0][0], outs[1][0]) < 5e-6 and rel(outs[0][1], outs[1][1]) < 5e-3


def _pair(**over):
    from dynaboa_amd import online as ON
    from dynaboa_amd.base_adaptor import synthetic_bundle
    mk = lambda: ON.OnlineAdaptor(ON.online_options(use_boa=1, interval=2, log_frames=4, **over),
                                  synthetic_bundle(seed=22, identity_pose=False, randomize_norm=True, smpl_seed=0), device="cuda:0")
    return ON, mk


def _frames(n, dev, offsets=(0, 100)):
    from dynaboa_amd import assets
    out = []
    for o in offsets:
        fr = {k: v.to(dev) for k, v in assets.make_online_frame(n + o, seed=22).items()}
        out.append((fr["image"], fr["smpl_j2d"], None))
    return out


def test_reload_of_one_sequence_leaves_the_others_of_its_group_alone():
    """The group's stepper is shared: reload() of sequence 0 resets ITS Adam step count, sequence 1 keeps count, moments and
    trajectory - its next frame equals that of a group nobody reloaded."""
    ON, mk = _pair()
    runs = []
    for reload0 in (True, False):
        grp = ON.OnlineGroup([mk(), mk()])
        a0, a1 = grp.adaptors
        for n in range(2):
            grp.step_processed(_frames(n, a0.device))
        ns = grp.group.stepper
        if reload0:
            theta0 = a0.model.module.theta.detach().clone()
            a0.reload()
            assert not torch.equal(a0.model.module.theta.detach(), theta0)
            assert float(a0.optimizer.state[a0.model.module.theta]["exp_avg"].abs().max()) == 0
        count = lambda r: int(ns.lib.dyb_stepper_get_i(ns.h, f"adam_step_{r}".encode()))
        assert count(0) == (0 if reload0 else 2) and count(1) == 2
        assert int(a0.optimizer.state[a0.model.module.theta]["step"]) == count(0)
        assert int(a1.optimizer.state[a1.model.module.theta]["step"]) == 2
        assert float(a1.optimizer.state[a1.model.module.theta]["exp_avg"].abs().max()) > 0
        before = a1.model.module.theta.detach().clone()
        res = grp.step_processed(_frames(2, a0.device))
        st1 = a1.optimizer.state[a1.model.module.theta]
        assert count(0) == (1 if reload0 else 3) and count(1) == 3 and int(st1["step"]) == 3
        runs.append(dict(d=(a1.model.module.theta.detach().double() - before.double()), m=st1["exp_avg"].clone(), cam=res[1]["cam"].clone(),
                         theta=a1.model.module.theta.detach().clone()))
    a, b = runs
    rel = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm())
    assert rel(a["d"], b["d"]) < 1e-3, rel(a["d"], b["d"])              # (a step taken with t = 1 bias corrections is 1.75 x as long)
    assert rel(a["theta"], b["theta"]) < 5e-6 and rel(a["m"], b["m"]) < 5e-3 and rel(a["cam"], b["cam"]) < 1e-5


def test_group_step_on_raw_frames_equals_the_sequences_alone():
    """OnlineGroup.step: frame + detection per sequence through dataprocess into one launch - each sequence's results are those of an
    OnlineAdaptor of its own on the same inputs; a sequence without a frame is refused before anything is filed."""
    ON, mk = _pair()
    rng = np.random.default_rng(11)
    grp, alone = ON.OnlineGroup([mk(), mk()]), [mk(), mk()]
    for n in range(3):
        frames = [rng.integers(0, 255, (120, 160, 3), dtype=np.uint8) for _ in range(2)]
        dets = [np.concatenate([rng.uniform(30, 110, (25, 2)), rng.uniform(0.2, 1.0, (25, 1))], 1).astype(np.float32) for _ in range(2)]
        got = grp.step(frames, dets)
        for r in range(2):
            want = alone[r].online_adaptation(frames[r], dets[r])
            assert torch.is_tensor(got[r]["bbox"]) and got[r]["bbox"].is_cuda and torch.equal(got[r]["bbox"], want["bbox"])
            for k in ("cam", "shape", "rotmat", "vts"):
                assert C.rel_err(got[r][k].detach().cpu().numpy().reshape(-1), want[k].detach().cpu().numpy().reshape(-1)) < 1e-5, (n, r, k)
    assert "ul/motion_loss" in grp.adaptors[1].fit_losses
    gs = [a.global_step for a in grp.adaptors]
    for bad in ([frames[0], None], [frames[0]]):
        with pytest.raises(ValueError, match="every sequence"):
            grp.step(bad, dets[:len(bad)])
    assert [a.global_step for a in grp.adaptors] == gs == [3, 3]


def test_frame_step_refuses_a_keypoint_set_out_of_range():
    """The option table stores any int; the frame step validates it: DYB_ERR_ARG with nothing launched (no frame step counted, the
    weights untouched), and the step runs once the value is valid again."""
    s = C.OnlineStream("boa_i2", "native")
    s.frame()
    ns = s.ad._native
    theta = s.hmr.theta.detach().clone()
    frames = ns.lib.dyb_stepper_get_f(ns.h, b"host_frames")
    assert ns.lib.dyb_stepper_set_i(ns.h, b"kp_set", 7) == 0
    from dynaboa_amd import assets
    fr = {k: v.to(s.ad.device) for k, v in assets.make_online_frame(1, seed=22).items()}
    gs, hist = s.ad.global_step, dict(s.ad.history)
    with pytest.raises(RuntimeError, match="bad argument"):
        s.ad.adapt_processed(fr["image"], fr["smpl_j2d"])
    torch.cuda.synchronize()
    assert ns.lib.dyb_stepper_get_f(ns.h, b"host_frames") == frames and torch.equal(s.hmr.theta.detach(), theta)
    assert ns.lib.dyb_stepper_set_i(ns.h, b"kp_set", 1) == 0
    s.ad.global_step, s.ad.history = gs, hist                     # (the refused call had already filed its frame)
    s.frame()                                                     # frame 1 against the golden, as if nothing had happened


def test_driver_writes_what_the_api_returns(tmp_path):
    """python -m dynaboa_amd.online: three PIL-written frames + a detections .npz; Pred_<n>.npz equal the API's results for the same
    inputs, the overlay PNGs (--save_video 1) equal render() of the same result."""
    from PIL import Image
    from dynaboa_amd import online as ON
    from dynaboa_amd.base_adaptor import synthetic_bundle
    rng = np.random.default_rng(5)
    fdir, odir = tmp_path / "frames", tmp_path / "out"
    fdir.mkdir()
    names, frames, kps = [], [], []
    for i in range(3):
        f = rng.integers(0, 255, (120, 160, 3), dtype=np.uint8)
        Image.fromarray(f).save(fdir / f"{i:03d}.png")
        names.append(f"{i:03d}.png"); frames.append(f)
        kps.append(np.concatenate([rng.uniform(30, 110, (25, 2)), rng.uniform(0.2, 1.0, (25, 1))], 1).astype(np.float32))
    np.savez(tmp_path / "det.npz", imgname=np.array(names), keypoints=np.stack(kps))
    bundle = lambda: synthetic_bundle(seed=22, identity_pose=False, randomize_norm=True, smpl_seed=0)
    o = ON.online_options(use_boa=1, interval=2, save_video=1, frames=str(fdir), detections=str(tmp_path / "det.npz"), out=str(odir), log_frames=4)
    written = ON.run_driver(o, assets_bundle=bundle(), device="cuda:0")
    assert [os.path.basename(p) for p in written] == ["Pred_0.npz", "Pred_1.npz", "Pred_2.npz"]
    ad = ON.OnlineAdaptor(ON.online_options(use_boa=1, interval=2, log_frames=4), bundle(), device="cuda:0")
    for i in range(3):
        res = ad.online_adaptation(frames[i], kps[i])
        z = np.load(written[i])
        assert set(z.files) == {"verts", "cam", "rotmat", "beta"}
        cam = res["cam"]
        cam_t = torch.stack([cam[:, 1], cam[:, 2], 2 * 5000.0 / (224 * cam[:, 0] + 1e-9)], dim=-1)
        assert np.array_equal(z["verts"], res["vts"].cpu().numpy()) and np.array_equal(z["cam"], cam_t.cpu().numpy())
        assert np.array_equal(z["rotmat"], res["rotmat"].cpu().numpy()) and np.array_equal(z["beta"], res["shape"].cpu().numpy())
        pic = np.array(Image.open(odir / f"Pred_{i}.png"))
        assert np.array_equal(pic, ad.render(res, frames[i]).cpu().numpy())
        assert (pic != frames[i]).any()                                                  # a mesh was drawn
