"""Closed-form second derivative of the frame-loss head (--hvp_head closed) on the CPU: the product kernels compiled for the host
(tests/emu) against the fp64 oracle, and the selection rules of the flag.  The MI355X runs the same cases in test_head_hvp_gpu.py."""
import ctypes
import logging
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import head_hvp_cases as H
from conftest import cosine


@pytest.fixture(scope="module")
def be():
    from backends import EmuBackend
    return EmuBackend()


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
def gmm():
    from dynaboa_amd import assets
    return assets.load_gmm_prior()


@pytest.mark.parametrize("B", [1, 3])
def test_stage_rot6d_jvp(be, B):
    H.case_stage_rot6d(be, B)


@pytest.mark.parametrize("B", [1, 3])
def test_stage_lbs_jvp(be, smpl_tabs, B):
    H.case_stage_lbs(be, smpl_tabs, B)


@pytest.mark.parametrize("B", [1, 3])
def test_stage_frame_losses_jvp(be, smpl_tabs, gmm, B):
    H.case_stage_losses(be, smpl_tabs, gmm, B)


@pytest.mark.parametrize("name", H.HEAD_CASES)
def test_head_hvp_matches_fp64_oracle_and_beats_difference_quotient(be, smpl_tabs, gmm, name):
    H.case_head(be, smpl_tabs, gmm, name)


def test_head_hvp_at_exact_identity(be, smpl_tabs, gmm):
    H.case_identity(be, smpl_tabs, gmm)


def test_head_hvp_losses_and_argument_errors(be, smpl_tabs, gmm):
    H.case_head_losses_and_errors(be, smpl_tabs, gmm)


def test_python_head_hvp_is_the_library_call(be, smpl_tabs, gmm):
    H.case_python_entry(be, smpl_tabs, gmm)


def test_rot6d_jvp_clamped_norms(be):
    H.case_rot6d_degenerate(be)


# ------------------------------------------------------------------------------------------------------------- selection rules
def test_hvp_head_defaults_to_fd():
    from dynaboa_amd import benchmark as DB
    assert DB.parser.parse_args([]).hvp_head == os.environ.get("DYB_HVP_HEAD", "fd")      # (unset: the child-process test below)
    assert DB.parser.parse_args(["--hvp_head", "closed"]).hvp_head == "closed"
    with pytest.raises(SystemExit):
        DB.parser.parse_args(["--hvp_head", "exact"])
    from dynaboa_amd import hvp
    with pytest.raises(ValueError):
        hvp.frame_level_hvp(None, None, None, None, None, None, 1.0, 1.0, 1.0, head="exact")


@pytest.mark.parametrize("value,expect", [("closed", "closed"), ("fd", "fd"), (None, "fd")])
def test_hvp_head_environment_default(value, expect):
    """The parser reads DYB_HVP_HEAD when the module is imported: checked in a child process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k != "DYB_HVP_HEAD"}
    if value is not None:
        env["DYB_HVP_HEAD"] = value
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    out = subprocess.run([sys.executable, "-c", "from dynaboa_amd import benchmark as DB; print(DB.parser.parse_args([]).hvp_head)"],
                         env=env, capture_output=True, text=True, cwd=root, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == expect


def test_closed_head_on_a_level_with_other_terms_keeps_fd_and_says_so_once(emu_lib, monkeypatch, caplog):
    """A level with teacher / motion / labelled terms has no closed form: under --hvp_head closed the whole level goes to the multi-pass
    form (difference quotient of its head), never to frame_level_hvp, and the log says so once per run."""
    from dynaboa_amd import assets, benchmark as DB, hvp
    from dynaboa_amd.base_adaptor import synthetic_bundle
    o = DB.frame_only_options(inner_step=1, second_order=1, hvp="exact", hvp_head="closed", use_temporal_losses_upper=1, use_meanteacher=1)
    ad = DB.Adaptor(o, synthetic_bundle(seed=22, identity_pose=True, randomize_norm=True), device="cpu")
    calls = []
    monkeypatch.setattr(hvp, "general_level_hvp", lambda *a, **k: calls.append("general") or (lambda v: v))
    monkeypatch.setattr(hvp, "frame_level_hvp", lambda *a, **k: calls.append(("frame", k.get("head"))) or (lambda v: v))
    batch = assets.make_frame(0, 1, seed=22)
    image, kp = batch["image"], batch["smpl_j2d"]
    learner = ad.model.clone()
    with caplog.at_level(logging.WARNING, logger="dynaboa_amd.base_adaptor"):
        for _ in range(3):
            ad.level_hvp_factory("upper", image, kp, learner)(ad.model.module.theta.detach())
    said = [r for r in caplog.records if "hvp_head closed" in r.getMessage()]
    assert len(said) == 1 and "difference quotient" in said[0].getMessage()
    assert calls == ["general"] * 3
    # the frame-loss level of the same run takes the closed head
    ad.level_hvp_factory("lower", image, kp, learner)(ad.model.module.theta.detach())
    assert calls[-1] == ("frame", "closed")


@pytest.mark.slow
def test_frame_level_closed_head_hvp_matches_oracle_second_derivative(emu_lib, gmm_t, monkeypatch):
    """The set-up of test_host_emu.test_frame_level_exact_hvp_matches_oracle_second_derivative with --hvp_head closed: H v of a whole
    frame-loss level against torch differentiating the oracle's level loss twice, per tensor, same bounds (relative 3e-3, cosine
    0.9999); the fd head's figures next to it.  That the product really went through dyb_head_hvp is counted (HeadSpy), and its result
    differs from the fd head's in the bits.  Which head is closer to the oracle cannot be told at this level: both sit at 1.0e-3, the
    backbone's fp32 error, three decades above either head's."""
    from oracle import ref_cpu as O
    from dynaboa_amd import assets, benchmark as DB
    from dynaboa_amd.base_adaptor import synthetic_bundle
    from dynaboa_amd.hmr import get_layout
    o = DB.frame_only_options(inner_step=1, second_order=1, hvp="exact", hvp_head="closed")
    ad = DB.Adaptor(o, synthetic_bundle(seed=22, identity_pose=True, randomize_norm=True), device="cpu")
    ad.model.eval()
    batch = assets.make_frame(0, 1, seed=22)
    image, kp = batch["image"], batch["smpl_j2d"]
    L = get_layout(1)
    theta = ad.model.module.theta.detach()
    mp = assets.make_smpl_mean_params(identity_pose=True, seed=3)
    sd = assets.make_synthetic_checkpoint(22, mp, randomize_norm=True, prefix="")["model"]
    oa = O.Adapter(sd, O.smpl_tables_to_torch(assets.make_synthetic_smpl(0)), gmm_t,
                   dict(retrieval=0, lower_level_mixtrain=0, upper_level_mixtrain=0, use_meanteacher=0, use_motion=0, dynamic_boa=0,
                        use_temporal_losses_upper=0, inner_step=1))
    names = list(oa.theta)
    plist = [oa.theta[k] for k in names]
    rng = np.random.default_rng(9)
    vdict = {k: torch.from_numpy(rng.standard_normal(tuple(oa.theta[k].shape)).astype(np.float32)) * (0.02 if oa.theta[k].dim() > 1 else 0.05)
             for k in names}

    def level(w):
        rot, shape, cam = O.hmr_forward(oa._full(w), image)
        j49, _ = oa.decode(rot, shape)
        return oa.frame_losses(rot, shape, O.projection(cam, j49), kp, "ll")
    g = torch.autograd.grad(level(oa.theta), plist, create_graph=True)
    gv = sum((a * vdict[k]).sum() for a, k in zip(g, names))
    hv_ref = dict(zip(names, torch.autograd.grad(gv, plist)))
    vfull = dict(vdict, **{k: torch.zeros_like(v) for k, v in oa.buf.items()})
    v = L.pack(vfull)
    learner = ad.model.clone()

    def errs(Hd):
        out = {}
        for k in names:
            b = hv_ref[k].double().flatten()
            if float(b.norm()) > 0:
                a = Hd[k].double().flatten()
                out[k] = (float((a - b).norm() / b.norm()), cosine(a.numpy(), b.numpy()))
        return out
    spy = H.HeadSpy(monkeypatch)
    hv_closed = ad.level_hvp_factory("lower", image, kp, learner)(theta)(v)
    spy.assert_closed(B=1)
    assert spy.n["products"] == 1
    ec = errs(L.unpack(hv_closed))
    ad.options.hvp_head = "fd"
    spy.reset()
    hv_fd = ad.level_hvp_factory("lower", image, kp, learner)(theta)(v)
    spy.assert_fd(B=1)
    assert not torch.equal(hv_closed, hv_fd)
    ef = errs(L.unpack(hv_fd))
    print("closed head: max rel %.2e  min cos %.7f | fd head: max rel %.2e  min cos %.7f" % (
        max(x[0] for x in ec.values()), min(x[1] for x in ec.values()), max(x[0] for x in ef.values()), min(x[1] for x in ef.values())))
    bad = {k: x for k, x in ec.items() if x[0] > 3e-3 or x[1] < 0.9999}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1][0])[:8]
