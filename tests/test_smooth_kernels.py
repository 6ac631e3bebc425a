"""dyb_smooth_sequences and dyb_one_euro_step (csrc/smooth.hip) against the fp64 NumPy restatement of their rules, through the cases of
tests/smooth_cases.py: on the kernel emulator and, marked gpu, on the device through the same C ABI."""
import numpy as np
import pytest

import smooth_cases as SM
from backends import EmuBackend, GpuBackend


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


@pytest.fixture(scope="module")
def gpu():
    return GpuBackend()


def test_inputs_keep_a_sign_margin_and_hold_a_sign_flip():
    """No (centre, tap) pair within 8 frames has |dot| below SIGN_MARGIN - no rounding can decide a sign - and the sign step is
    exercised: joint 0 crosses the angle pi, where rot_to_quat's result changes sign between neighbouring frames."""
    x = SM.make_inputs()
    low, flips = SM.sign_margin(x["rotmat"], SM.LENGTHS, reach=8)
    print("sign margin", low, "adjacent sign flips", flips)
    assert low >= SM.SIGN_MARGIN and flips >= 1
    low, flips = SM.sign_margin(SM.oe_stream()[0].swapaxes(0, 1).reshape(-1, SM.J, 9), (SM.OE_STEPS,) * SM.OE_R, reach=1)
    assert low >= SM.SIGN_MARGIN


def test_measured_floors():
    """The float32 against the float64 evaluation of the restatement: the floors the bounds are 8 x of."""
    f, g = SM.measure_floor(), SM.measure_oe_floor()
    print("window floor", f, "one-euro floor", g)
    assert SM.FLOOR / 2 < f <= SM.FLOOR and SM.OE_FLOOR / 2 < g <= SM.OE_FLOOR
    assert SM.BOUND == 8 * SM.FLOOR and SM.OE_BOUND == 8 * SM.OE_FLOOR


def test_restatement_reduces_the_jitter():
    x = SM.make_inputs()
    ref = SM.ref_smooth(x["rotmat"], x["betas"], x["cam"], SM.LENGTHS, SM.gaussian(4, 2.0), 4)[0]
    assert SM.accel_ratio(x["rotmat"], ref, x["clean_rotmat"], SM.LENGTHS) >= 10.0


WINDOW_CASES = ["channels", "tile_boundary", "masks", "copies", "nonfinite_taps", "determinism", "position_independence", "arguments",
                "purpose", "oe_stream", "oe_closed_form", "oe_arguments"]


@pytest.mark.parametrize("h", [1, 4, 8, 32])
def test_batch_emu(emu, h):
    SM.case_batch(emu, h)


@pytest.mark.parametrize("case", WINDOW_CASES)
def test_case_emu(emu, case):
    getattr(SM, "case_" + case)(emu)


@pytest.mark.gpu
@pytest.mark.parametrize("h", [1, 4, 8, 32])
def test_batch_gpu(gpu, h):
    SM.case_batch(gpu, h)


@pytest.mark.gpu
@pytest.mark.parametrize("case", WINDOW_CASES)
def test_case_gpu(gpu, case):
    getattr(SM, "case_" + case)(gpu)
