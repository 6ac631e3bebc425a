"""dyb_track_videos (csrc/track.hip) against the fp64 NumPy restatement of its rule, through the cases of tests/track_cases.py: on the
kernel emulator and, marked gpu, on the device through the same C ABI."""
import numpy as np
import pytest

import track_cases as TR
from backends import EmuBackend, GpuBackend


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


@pytest.fixture(scope="module")
def gpu():
    return GpuBackend()


def test_scene_conditions():
    """The conditions under which ids are compared for equality, on the float64 restatement: candidate similarities of one frame at
    least MARGIN apart, none within MARGIN of s_min; the measured fp32 / fp64 floor at most MARGIN / 100 and inside (FLOOR / 2,
    FLOOR]; and the scene holds what it is meant to: at least 3 ambiguous frames, 7 tracks of one person each, an id kept over the
    3-frame gap, a new id after the 20-frame gap, a person entering at frame 15."""
    c = TR.scene_conditions()
    print(c)
    assert c["gap"] >= TR.MARGIN and c["edge"] >= TR.MARGIN
    assert c["floor"] <= TR.MARGIN / 100 and TR.FLOOR / 2 < c["floor"] <= TR.FLOOR <= TR.MARGIN / 100 and TR.BOUND == 8 * TR.FLOOR
    assert c["ids_equal"] and c["pure"] and c["tracks"] == 7 and c["untrackable"] == 1 and c["ambiguous"] >= 3
    assert c["short_gap"][0] == c["short_gap"][1] and c["long_gap"][0] != c["long_gap"][1] and c["long_gap"][1] > c["enters"] >= 5


def test_restatement_defaults_are_the_python_defaults():
    from dynaboa_amd import internet as I, track as T
    assert TR.RULE == dict(c_min=T.C_MIN, kappa=T.KAPPA, s_min=T.S_MIN, max_age=T.MAX_AGE, min_common=T.MIN_COMMON)
    assert T.C_MIN == I.CONF_THRESHOLD
    assert (T.MAX_PEOPLE, T.MAX_KP) == (TR.MAX_PEOPLE, TR.MAX_KP)


CASES = ["scene", "frame_ids", "ties", "limits", "thresholds", "determinism", "arguments"]


@pytest.mark.parametrize("case", CASES)
def test_case_emu(emu, case):
    getattr(TR, "case_" + case)(emu)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_case_gpu(gpu, case):
    getattr(TR, "case_" + case)(gpu)
