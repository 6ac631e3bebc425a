"""Host level of the online path (dynaboa_amd/online.py) on the CPU: dataprocess against the reference's recorded values, the history
lag and the motion gate, the refusals, reload() - with the emulator build of the library where one is needed."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import online_ref as R
from conftest import golden


@pytest.fixture(scope="module")
def emu_lib():
    from emu.build_emu import build
    from dynaboa_amd import _abi, _lib
    lib = _abi.bind(ctypes.CDLL(build()))
    saved = _lib._lib
    _lib.use_library(lib)
    yield lib
    _lib._lib = saved


@pytest.fixture(scope="module")
def adaptor(emu_lib):
    from dynaboa_amd import online as ON
    from dynaboa_amd.base_adaptor import synthetic_bundle
    return ON.OnlineAdaptor(ON.online_options(use_boa=1, interval=2, log_frames=4),
                            synthetic_bundle(seed=22, identity_pose=False, randomize_norm=True), device="cpu")


@pytest.mark.parametrize("case", ["full", "missing", "straddle"])
@pytest.mark.parametrize("sf", [1.0, 1.2])
def test_dataprocess_matches_the_reference_exactly(case, sf):
    """bbox over ALL 25 rows (undetected (0, 0, 0) rows included), scale = scaleFactor * max(w, h) / 200, confidence > 0.3, keypoints
    through the integer-rounding transform: golden g9_online_dataprocess (the reference's own dataprocess), bit for bit."""
    from dynaboa_amd import online as ON
    g = golden("g9_online_dataprocess.npz")
    kp_in = g[f"{case}_in"]
    center, scale, bbox = ON.bbox_center_scale(kp_in, sf)
    kp = ON.process_keypoints(kp_in, center, scale)
    assert np.array_equal(bbox[None, :], g[f"{case}_bbox_{sf}"])
    assert kp.dtype == np.float32 and np.array_equal(kp[None], g[f"{case}_kp_{sf}"])
    assert set(np.unique(kp[:, 2])) <= {0.0, 1.0}
    if case == "missing":
        assert kp_in[:, 0].min() == 0.0 and bbox[0] == kp_in[:, 0].max() / 2 and bbox[1] == kp_in[:, 1].max() / 2     # the undetected rows pull the box to the origin
        assert (kp[[3, 11, 24], 2] == 0).all()
    if case == "straddle":
        assert kp[:, 2].tolist() == [float(c > 0.3) for c in kp_in[:, 2]] and 0 < kp[:, 2].sum() < 25


def test_dataprocess_returns_the_layout_the_kernels_read(adaptor):
    g = golden("g9_online_dataprocess.npz")
    frame = np.random.default_rng(0).integers(0, 255, (480, 640, 3), dtype=np.uint8)
    image, kp49, bbox = adaptor.dataprocess(frame, g["full_in"].astype(np.float32), scaleFactor=1.2)
    assert image.shape == (1, 3, 224, 224) and kp49.shape == (1, 49, 3) and bbox.shape == (1, 3)
    assert np.array_equal(kp49[0, :25].numpy(), g["full_kp_1.2"][0]) and float(kp49[0, 25:].abs().max()) == 0       # detections in slots 0..24
    assert torch.is_tensor(bbox) and bbox.dtype == torch.float32 and np.array_equal(bbox.numpy(), g["full_bbox_1.2"].astype(np.float32))
    with pytest.raises(ValueError):
        adaptor.dataprocess(frame, np.zeros((24, 3)))


@pytest.mark.parametrize("interval", [1, 2, 5])
def test_history_lag_and_motion_gate_follow_the_reference(emu_lib, interval):
    """save_hist increments global_step BEFORE the adaptation: frame n stores history[n], the motion term is on iff n >= interval and
    reads frame n + 1 - interval (interval - 1 frames back) - for 6 frames, through the code the frame step itself asks."""
    from dynaboa_amd import online as ON
    ad = ON.OnlineAdaptor.__new__(ON.OnlineAdaptor)
    ad.options = ON.schedule_options(ON.online_options(use_boa=1, interval=interval))
    ad.history, ad.global_step, ad.bundle = {}, 0, SimpleNamespace()
    seen = []
    for n in range(6):
        img, kp = torch.full((1, 1), float(n)), torch.full((1, 1), float(100 + n))
        ad.save_hist(img, kp)
        assert ad.global_step == n + 1 and n in ad.history
        hist, ex = ad._native_full_inputs(dict(image=img, smpl_j2d=kp))                            # what the native stepper is handed
        assert ex is None
        seen.append(None if hist is None else (int(hist[0].item()), int(hist[1].item()) - 100))
        # the autograd composition: BaseAdaptor._level asks motion_on() and, where it is on, _motion_term reads get_hist()
        on, h = R.history_rule(n, interval)
        assert ad.motion_on() == on == (hist is not None), (n, interval)
        if on:
            assert (int(ad.get_hist()[0].item()), int(ad.get_hist()[1].item()) - 100) == (h, h)
        assert len(ad.history) <= max(interval, 1)                                                 # pruned, never short
    want = []
    for n in range(6):
        on, h = R.history_rule(n, interval)
        assert on == (n >= interval)
        want.append((h, h) if on else None)
    assert seen == want, (seen, want)
    if interval == 2:
        assert seen == [None, None, (1, 1), (2, 2), (3, 3), (4, 4)]


def test_refusals(adaptor):
    from dynaboa_amd import losses as LS, online as ON
    so = SimpleNamespace(kp_set="op25", second_order=1, hvp_head="fd")
    closed = SimpleNamespace(kp_set="op25", second_order=0, hvp_head="closed")
    assert "second_order" in LS.kp_set_refusal(so) and "gt24" in LS.kp_set_refusal(so)
    assert "hvp_head closed" in LS.kp_set_refusal(closed)
    assert LS.kp_set_refusal(SimpleNamespace(kp_set="gt24", second_order=1, hvp_head="closed")) is None
    assert LS.kp_set_refusal(SimpleNamespace(kp_set="op25", second_order=0, hvp_head="fd")) is None
    with pytest.raises(ValueError, match="unknown keypoint set"):
        LS.kp_set_refusal(SimpleNamespace(kp_set="coco17"))
    # the level code asks before it computes anything
    saved = adaptor.options.second_order
    adaptor.options.second_order = 1
    try:
        with pytest.raises(ValueError, match="second_order with kp_set op25"):
            adaptor._level("lower", torch.zeros(1, 3, 224, 224), torch.zeros(1, 49, 3), None, adaptor.model)
    finally:
        adaptor.options.second_order = saved
    adaptor.options.hvp_head = "closed"
    try:
        with pytest.raises(ValueError, match="hvp_head closed with kp_set op25"):
            adaptor._level("upper", torch.zeros(1, 3, 224, 224), torch.zeros(1, 49, 3), None, adaptor.model)
    finally:
        adaptor.options.hvp_head = "fd"
    with pytest.raises(ValueError):
        ON.online_options(no_such_flag=1)


def test_frame_step_refuses_a_keypoint_set_out_of_range(adaptor):
    """kp_set is an int row of the option table (the setter stores anything); the frame step returns DYB_ERR_ARG before its first launch."""
    from dynaboa_amd import native_step as NS
    ns = NS.NativeStepper(adaptor, 2)
    assert ns.full and int(ns.lib.dyb_stepper_get_i(ns.h, b"kp_set")) == 1 and int(ns.lib.dyb_stepper_get_i(ns.h, b"metrics")) == 0
    assert ns.lib.dyb_stepper_set_i(ns.h, b"kp_set", 2) == 0 and int(ns.lib.dyb_stepper_get_i(ns.h, b"kp_set")) == 2
    theta = adaptor.model.module.theta.detach().clone()
    batch = dict(image=torch.zeros(1, 3, 224, 224), smpl_j2d=torch.zeros(1, 49, 3))
    with pytest.raises(RuntimeError, match="bad argument"):
        ns.adapt_frame_full(batch)
    assert ns.lib.dyb_stepper_get_f(ns.h, b"host_frames") == 0.0 and ns.frame == 0
    assert torch.equal(adaptor.model.module.theta.detach(), theta)


def test_reload_restores_checkpoint_and_fresh_adam(adaptor):
    ad = adaptor
    hmr = ad.model.module
    theta0, teacher0 = hmr.theta.detach().clone(), ad.teacher.theta.detach().clone()
    st = ad.optimizer.state.get(hmr.theta)
    if not st:
        st = ad.optimizer.state[hmr.theta] = dict(step=0, exp_avg=torch.zeros_like(hmr.theta), exp_avg_sq=torch.zeros_like(hmr.theta))
    with torch.no_grad():
        hmr.theta.add_(0.5); ad.teacher.theta.mul_(0.5)
    st["exp_avg"].fill_(1.0); st["exp_avg_sq"].fill_(2.0); st["step"] = 7
    ad.history[3], ad.global_step = dict(image=None, s2d=None), 4
    m_ptr = st["exp_avg"].data_ptr()
    ad.reload()
    assert torch.equal(hmr.theta.detach(), theta0) and torch.equal(ad.teacher.theta.detach(), teacher0)
    st = ad.optimizer.state[hmr.theta]
    assert st["step"] == 0 and float(st["exp_avg"].abs().max()) == 0 and float(st["exp_avg_sq"].abs().max()) == 0
    assert st["exp_avg"].data_ptr() == m_ptr                      # in place: a stepper bound to these moments keeps addressing them
    assert ad.global_step == 4 and 3 in ad.history                # history and the step counter stay, as in the reference
    ad.history.clear(); ad.global_step = 0


def test_reload_without_boa(emu_lib):
    """use_boa 0: the model is the plain network (no fast-weight wrapper) - reload() takes the checkpoint without the wrapper's prefix."""
    from dynaboa_amd import online as ON
    from dynaboa_amd.base_adaptor import synthetic_bundle
    ad = ON.OnlineAdaptor(ON.online_options(use_boa=0, log_frames=4), synthetic_bundle(seed=22, identity_pose=False, randomize_norm=True), device="cpu")
    ps = list(ad.model.parameters())
    before = [p.detach().clone() for p in ps]
    for p in ps:
        with torch.no_grad():
            p.add_(0.25)
        ad.optimizer.state[p] = dict(step=3, exp_avg=torch.ones_like(p), exp_avg_sq=torch.ones_like(p))
    ad.global_step = 2
    ad.reload()
    for p, b in zip(ps, before):
        st = ad.optimizer.state[p]
        assert torch.equal(p.detach(), b) and st["step"] == 0 and float(st["exp_avg"].abs().max()) == 0 and float(st["exp_avg_sq"].abs().max()) == 0
    assert ad.global_step == 2
