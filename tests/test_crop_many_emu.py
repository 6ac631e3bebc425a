"""The many-crop entry of csrc/preprocess.hip (``dyb_crop_resize_normalize_many``) on the kernel emulator: every output bit-identical
to the single-crop entry called for that crop alone, the error returns, and ``datasets.preprocess_frames`` against the oracle.
Cases and helpers: tests/crop_many_cases.py (the same ones run on cuda:0 in tests/test_crop_many_gpu.py)."""
import ctypes

import pytest

import crop_many_cases as CM


@pytest.fixture(scope="module")
def emu_lib():
    from emu.build_emu import build
    from dynaboa_amd import _abi, _lib
    lib = _abi.bind(ctypes.CDLL(build()))
    saved = _lib._lib
    _lib.use_library(lib)
    yield lib
    _lib._lib = saved


@pytest.mark.parametrize("name", list(CM.BOX_CASES) + ["n64"])
def test_many_equals_single_bit_for_bit(emu_lib, name):
    CM.run_box_case(emu_lib, name, "cpu")


def test_error_returns_leave_outputs_untouched(emu_lib):
    CM.check_error_returns(emu_lib, "cpu")


def test_preprocess_frames_against_single_and_oracle(emu_lib):
    CM.check_python_entry("cpu")


def test_preprocess_frames_chunks_above_64(emu_lib):
    CM.check_python_entry("cpu", reps=14)                 # 70 crops: a call of 64 and a call of 6


def test_preprocess_frames_rejects_bad_input(emu_lib):
    import numpy as np
    import torch
    from dynaboa_amd import datasets as D
    img = torch.from_numpy(CM.frame(*CM.F_A))
    with pytest.raises(ValueError):
        D.preprocess_frames([img.float()], [np.array([30.0, 20.0])], [0.2], res=16)
    with pytest.raises(ValueError):
        D.preprocess_frames([img], [np.array([30.0, 20.0])], [0.2, 0.3], res=16)
    with pytest.raises(ValueError):
        D.preprocess_frames([img], [np.array([30.0, 20.0])], [0.2], res=16, out=torch.empty(2, 3, 16, 16))
