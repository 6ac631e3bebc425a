"""dyb_rows_inv_norm / dyb_kmeans_assign / dyb_kmeans_update (csrc/kmeans.hip) against the fp64 NumPy restatements of
tests/kmeans_cases.py: on the kernel emulator and, marked gpu, on the device through the same C ABI.  Assignments, counts and `changed`
are exact (the inputs are decided by at least MARGIN, asserted below); cosines and centres are held to bounds derived from the number of
fp32 roundings."""
import numpy as np
import pytest

import kmeans_cases as KC
from backends import EmuBackend, GpuBackend

PADDED = ((130, 33, 64), (65, 67, 2048))       # (N, K, D) run again with a row pitch of D + 8 floats, the padding NaN


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


@pytest.fixture(scope="module")
def gpu():
    return GpuBackend()


def test_inputs_are_decided_by_a_margin():
    """Every row of every assign shape has an fp64 gap of at least MARGIN between its best and second-best cosine, so no fp32
    summation order can decide an assignment; the same for the tie case's rows against every OTHER value, and for every decision
    (assignments at each iteration, the reseed's row against the runner-up) of the three designed k-means runs."""
    for N in KC.NS:
        for K in KC.KS[1:]:
            for D in KC.DS:
                x, centers, targets = KC.assign_inputs(N, K, D)
                arg, _, gap = KC.argmax_margin(KC.cosines64(x, centers))
                assert gap.min() >= KC.MARGIN, (N, K, D, gap.min())
    x, _ = KC.blob_data()
    runs = {name: KC.lloyd64(x, init) for name, init in KC.blob_inits().items()}
    for name, r in runs.items():
        assert min(r["margins"]) >= KC.MARGIN and all(m >= KC.MARGIN for m in r["reseed_margins"]), name
    assert (runs["one_per_blob"]["iterations"], runs["one_per_blob"]["reseeds"]) == (2, 0)
    assert (runs["two_in_one"]["iterations"], runs["two_in_one"]["reseeds"]) == (2, 0)
    assert np.bincount(runs["two_in_one"]["assign"][-1]).tolist() == [30, 30, 120, 60, 60]        # a local optimum: blob 0 stays split
    assert (runs["away"]["iterations"], runs["away"]["reseeds"]) == (3, 1) and len(runs["away"]["reseed_margins"]) == 1
    assert np.bincount(runs["away"]["assign"][0]).tolist() == [60, 60, 1, 119, 60]                # the reseed took one row of blob 2


def _inv_norm(be):
    for N, D, pad in ((1, 32, 0), (5, 64, 0), (130, 2048, 0), (7, 96, 4)):
        KC.check_inv_norm(be, N, D, pad)


def _assign(be, K, D):
    for N in KC.NS:
        KC.check_assign(be, N, K, D)


def _padded(be):
    for N, K, D in PADDED:
        KC.check_assign(be, N, K, D, pad=KC.PAD)
        KC.check_update(be, N, K, D, "random", pad=KC.PAD)
    for N, K, D in KC.UPDATE_EXTRA:
        for mode in ("random", "one"):
            KC.check_update(be, N, K, D, mode)
    KC.check_assign(be, 70, 3, 96)                 # an odd number of 32-float steps


def _update(be, K, D):
    for N in KC.NS:
        for mode in ("random", "one"):
            KC.check_update(be, N, K, D, mode)


def test_inv_norm_emu(emu):
    _inv_norm(emu)


@pytest.mark.parametrize("D", KC.DS)
@pytest.mark.parametrize("K", KC.KS)
def test_assign_emu(emu, K, D):
    _assign(emu, K, D)


def test_assign_tie_errors_padding_and_chunks_emu(emu):
    for D in KC.DS:
        KC.check_assign_tie(emu, D)
    KC.check_assign_errors(emu)
    _padded(emu)


@pytest.mark.parametrize("D", KC.DS)
@pytest.mark.parametrize("K", KC.KS)
def test_update_emu(emu, K, D):
    _update(emu, K, D)


@pytest.mark.gpu
def test_inv_norm_gpu(gpu):
    _inv_norm(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("D", KC.DS)
def test_assign_gpu(gpu, D):
    for K in KC.KS:
        _assign(gpu, K, D)


@pytest.mark.gpu
def test_assign_tie_errors_padding_and_chunks_gpu(gpu):
    for D in KC.DS:
        KC.check_assign_tie(gpu, D)
    KC.check_assign_errors(gpu)
    _padded(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("D", KC.DS)
def test_update_gpu(gpu, D):
    for K in KC.KS:
        _update(gpu, K, D)
