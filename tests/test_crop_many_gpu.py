"""tests/test_crop_many_emu.py's cases on cuda:0: ``dyb_crop_resize_normalize_many`` bit-identical to the single-crop entry on the
device, and back-to-back calls of ``datasets.preprocess_frames`` with different boxes (more calls than the staging ring has blocks,
nothing synchronising in between) each keeping their own descriptors."""
import numpy as np
import pytest
import torch

import crop_many_cases as CM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from dynaboa_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("name", list(CM.BOX_CASES) + ["n64"])
def test_many_equals_single_bit_for_bit_gpu(lib, name):
    CM.run_box_case(lib, name, "cuda:0")


def test_error_returns_leave_outputs_untouched_gpu(lib):
    CM.check_error_returns(lib, "cuda:0")


def test_preprocess_frames_against_single_and_oracle_gpu(lib):
    CM.check_python_entry("cuda:0")
    CM.check_python_entry("cuda:0", reps=14)


def test_back_to_back_calls_keep_their_staging_gpu(lib):
    """20 calls in a row (the ring has 8 blocks), each with other boxes and another crop count, no synchronisation until all are
    enqueued: every call's outputs equal the single entry's."""
    from dynaboa_amd import datasets as D
    dev = torch.device("cuda:0")
    frames = [torch.from_numpy(CM.frame(*CM.F_A)).to(dev), torch.from_numpy(CM.frame(*CM.F_B)).to(dev)]
    rng = np.random.default_rng(9)
    calls, outs = [], []
    for k in range(20):
        n = 1 + k % 5
        which = [int(v) for v in rng.integers(0, 2, n)]
        cs = [(np.array([rng.uniform(5, 55), rng.uniform(5, 35)]), float(rng.uniform(0.08, 0.5))) for _ in range(n)]
        calls.append((which, cs))
    torch.cuda.synchronize()
    for which, cs in calls:
        outs.append(D.preprocess_frames([frames[w] for w in which], [c for c, _ in cs], [s for _, s in cs], res=16))
    torch.cuda.synchronize()
    for (which, cs), got in zip(calls, outs):
        for i, (w, (c, s)) in enumerate(zip(which, cs)):
            assert torch.equal(got[i], D.preprocess_frame(frames[w], c, s, res=16))
