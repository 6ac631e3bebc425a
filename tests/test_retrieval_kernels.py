"""dyb_retrieve_select / dyb_exemplar_gather (csrc/retrieval.hip) against an independent fp64 / NumPy check with its own
Philox-4x32-10 (tests/retrieval_cases.py): on the kernel emulator and, marked gpu, on the device through the same C ABI."""
import numpy as np
import pytest

import retrieval_cases as RC
from backends import EmuBackend, GpuBackend

KS = (1, 3, 17, 67)            # 17 and 67: more centres than one workgroup's chunk (16 by default, 5 as the second geometry)
CHUNKS = (0, 5)


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


@pytest.fixture(scope="module")
def gpu():
    return GpuBackend()


def test_row_generator_margin():
    """The rows the cases are built from are decided by far more than fp32 rounding: every row's fp64 gap between the best and the
    second-best cosine is at least MARGIN, for every shape the select cases use."""
    for K in KS[1:]:
        for nrep, active in RC.REPLICA_SETS.values():
            rng = np.random.default_rng(1000 * K + nrep)
            centers, inv, index = RC.make_bank(K, rng)
            targets = [int(rng.integers(0, K)) for _ in active]
            for x, t in zip(RC.make_rows(centers, targets, rng), targets):
                c, _, margin = RC.expected_pick(x, centers, inv, index, 0, 1)
                assert c == t and margin >= RC.MARGIN
    # the independent generator against the published Philox4x32-10 known-answer vectors (Random123 kat_vectors)
    assert RC.philox4x32_10([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert RC.philox4x32_10([0xffffffff] * 4, [0xffffffff] * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert RC.philox4x32_10([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def _select_all(be):
    for reps in RC.REPLICA_SETS:
        for K in KS:
            first = None
            for chunk in CHUNKS:
                picks = RC.case_select(be, K, reps, chunk)
                assert first is None or np.array_equal(first, picks)        # the same answers for both launch geometries
                first = picks


@pytest.mark.parametrize("reps", list(RC.REPLICA_SETS))
@pytest.mark.parametrize("K", KS)
def test_select_emu(emu, K, reps):
    a = RC.case_select(emu, K, reps, 0)
    b = RC.case_select(emu, K, reps, 5)
    assert np.array_equal(a, b)


def test_select_tie_and_errors_emu(emu):
    for chunk in CHUNKS:
        RC.case_tie_lowest_index(emu, chunk)
    RC.case_select_errors(emu)


def test_gather_emu(emu):
    RC.case_gather(emu)


@pytest.mark.gpu
def test_select_gpu(gpu):
    _select_all(gpu)


@pytest.mark.gpu
def test_select_tie_and_errors_gpu(gpu):
    for chunk in CHUNKS:
        RC.case_tie_lowest_index(gpu, chunk)
    RC.case_select_errors(gpu)


@pytest.mark.gpu
def test_gather_gpu(gpu):
    RC.case_gather(gpu)
