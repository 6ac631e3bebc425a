"""The online path (OpenPose BODY_25 detections, reference dynaboa_webcam.py) on the MI355X: the keypoint-set window of the loss kernels
through the C ABI on cuda:0, against torch-CPU autograd of the reference's formulas (tests/online_ref.py)."""
import pytest

import online_cases as C
from conftest import golden

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
def test_frame_head_op25(be, gmm, B):
    C.case_frame_op25(be, gmm, B)


@pytest.mark.parametrize("B", [1, 3])
def test_frame_head_op25_slot_24_alone(be, gmm, B):
    """Confidence 1 on slot 24 only - the 25th joint of a window whose staging arrays used to hold 24."""
    C.case_frame_op25(be, gmm, B, seed=12, conf="slot24")


def test_frame_head_op25_ignores_the_gt24_slots(be, gmm):
    C.case_frame_op25(be, gmm, 2, seed=13, conf="gt_only")


def test_frame_head_gt24_bit_identical_through_the_new_export(be, gmm):
    C.case_frame_gt24_bit_identical(be, golden, gmm)


@pytest.mark.parametrize("B", [1, 2])
def test_motion_term_op25(be, B):
    C.case_motion_op25(be, B)


def test_two_replicas_in_one_launch_equal_their_launches_alone(be, gmm):
    C.case_replicas(be, gmm)


def test_unknown_keypoint_set_is_refused_before_any_launch(be, gmm):
    C.case_unknown_set(be, gmm)
