"""SMPLify on the CPU: the kernels of csrc/smplify.hip and the one-call fit on the host build of the product sources (tests/emu),
against fp64 autograd, torch.optim.Adam and the goldens g12_smplify_* (tests/smplify_cases.py states the bounds)."""
import pytest

import smplify_cases as C
from conftest import golden


@pytest.fixture(scope="module")
def be():
    from backends import EmuBackend
    return EmuBackend()


@pytest.fixture(scope="module")
def gmm():
    from dynaboa_amd import assets
    return assets.load_gmm_prior()


@pytest.fixture(scope="module")
def heads():
    return golden("g12_smplify_heads.npz")


@pytest.fixture(scope="module")
def fit():
    return golden("g12_smplify_fit.npz")


@pytest.mark.parametrize("n", [1, 64, 65, 72])
def test_rodrigues_bwd_against_fp64_autograd(be, n):
    C.case_rodrigues_bwd(be, n)


@pytest.mark.parametrize("sel", [[0], [1], [0, 1, 2]], ids=["op_torso", "gt_torso", "B3"])
def test_camera_loss_against_the_reference(be, heads, sel):
    C.case_camera_loss(be, heads, sel)


@pytest.mark.parametrize("ignore", [0, 1])
@pytest.mark.parametrize("sel", [[1], [0, 1, 2]], ids=["B1", "B3"])
def test_body_loss_against_the_reference(be, heads, gmm, sel, ignore):
    C.case_body_loss(be, heads, gmm, sel, ignore)


def test_adam_against_torch(be):
    C.case_adam(be)


@pytest.mark.parametrize("iters", [0, 1])
def test_fit_against_the_reference(be, fit, smpl_tabs, gmm, iters):
    """B = 2: the ground-truth-torso sample and the one with a joint at exactly zero (the emulated LBS is slow: no longer loop here)."""
    C.case_fit(be, fit, smpl_tabs, gmm, [1, 2], iters)


def test_golden_margins(fit):
    C.check_margins(fit)


# ---- the Python surface on the host build (dynaboa_amd._lib.use_library): what tests/test_smplify_gpu.py runs on the device
@pytest.fixture()
def emu_python(be):
    from dynaboa_amd import _lib
    saved = _lib._lib
    _lib.use_library(be.lib)
    yield
    _lib._lib = saved


@pytest.mark.parametrize("native", [True, False], ids=["native", "composition"])
def test_fitter_one_iteration(emu_python, fit, smpl_tabs, native):
    C.case_fitter(smpl_tabs, fit, "cpu", native, 1, sel=(1, 2))


def test_rodrigues_has_a_gradient_in_composition(emu_python):
    C.case_rodrigues_autograd("cpu")


def test_refine_bridge(emu_python, fit, smpl_tabs):
    C.case_refine(smpl_tabs, fit, "cpu")


def test_get_fitting_loss_is_the_fit_s_last_evaluation(emu_python, fit, smpl_tabs):
    C.case_get_fitting_loss(smpl_tabs, fit, "cpu")
