"""Closed-form second derivative of the frame-loss head (--hvp_head closed) on the MI355X: the cases of head_hvp_cases.py on the real
library, and the benchmarked second-order stream with the closed head against the reference's second-order golden."""
import numpy as np
import pytest

import head_hvp_cases as H
from conftest import cosine, golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from backends import GpuBackend
    return GpuBackend()


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


def test_second_order_inner3_closed_head_matches_reference_second_order(monkeypatch):
    """The pattern of test_adaptation_gpu.test_second_order_inner3_exact_hvp_matches_reference_second_order with --hvp_head closed,
    against golden g5_so_inner3_frameonly, same bounds: upper loss 1e-4, gradient-norm error median 5e-4 / max 3e-3, slice cosine
    0.9999.  Every Hessian-vector product of the frame is counted through dyb_head_hvp (HeadSpy): three inner steps, one each."""
    from dynaboa_amd import assets, benchmark as DB
    from dynaboa_amd.base_adaptor import synthetic_bundle
    gso, gfo = golden("g5_so_inner3_frameonly.npz"), golden("g5_fo_inner3_frameonly.npz")
    o = DB.frame_only_options(inner_step=3, second_order=1, hvp="exact", hvp_head="closed")
    o.deferred_metrics = 0
    ad = DB.Adaptor(o, synthetic_bundle(seed=22, identity_pose=False, randomize_norm=True, smpl_seed=0), device="cuda:0")
    ad.reset_records(1)
    hmr = ad.model.module
    ad.global_step = 0
    ad.fit_losses = {}
    batch = {k: v.to(ad.device) for k, v in assets.make_frame(0, 1, seed=22).items()}
    ad.model.eval()
    spy = H.HeadSpy(monkeypatch)
    ad.adaptation(batch)
    spy.assert_closed(B=1)
    assert spy.n["products"] == 3, spy.n
    up = float(ad.fit_losses["ul/total"])
    assert abs(up - gso["upper_loss"][0]) < 1e-4 * abs(gso["upper_loss"][0])
    st = ad.optimizer.state[hmr.theta]
    g1 = hmr._layout1.unpack((st["exp_avg"] / (1 - ad.options.beta1)).cpu())
    names = [str(x) for x in gso["names"]]
    gn = np.array([float(g1[k].double().norm()) for k in names])
    err = np.abs(gn - gso["g1_norms"]) / gso["g1_norms"]
    gap = np.abs(gfo["g1_norms"] - gso["g1_norms"]) / gso["g1_norms"]
    sl = {k[3:]: cosine(g1[k[3:]].flatten()[:256].numpy(), gso[k]) for k in gso.files if k.startswith("g1_") and k != "g1_norms"}
    print("closed-head SO inner3: grad-norm error median %.2e max %.2e (FO-SO gap median %.2e), min slice cosine %.6f" % (
        np.median(err), err.max(), np.median(gap), min(sl.values())))
    assert np.median(err) < 5e-4 and err.max() < 3e-3
    assert min(sl.values()) > 0.9999, sl
