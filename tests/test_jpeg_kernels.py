"""dyb_jpeg_encode_many (csrc/jpeg.hip) against the NumPy restatement of its rules in tests/jpeg_cases.py - which tests/test_jpeg_host.py
pins to the scans PIL writes - on the kernel emulator and, marked gpu, on the device through the same C ABI."""
import pytest

import jpeg_cases as J
from backends import EmuBackend, GpuBackend


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


@pytest.fixture(scope="module")
def gpu():
    return GpuBackend()


def test_case_set_covers_the_coder():
    """Asserted on the restatement, over the sizes x contents x qualities x subsamplings of the equality cases alone."""
    st = J.coverage()
    print(sorted(st.dc_cat), sorted(st.ac_size), st.zrl, st.eob, st.no_eob, st.stuffed, st.ends_stuffed)
    assert st.dc_cat == set(range(12))
    assert st.ac_size >= set(range(1, 11))
    assert st.zrl >= 1 and st.eob >= 1 and st.no_eob >= 1
    assert st.stuffed >= 100 and st.ends_stuffed >= 1


EQUAL = [(c, s, q) for c in J.CONTENTS for s in J.SUBSAMPLINGS for q in J.QUALITIES]


@pytest.mark.parametrize("content,subsampling,quality", EQUAL)
def test_equal_emu(emu, content, subsampling, quality):
    J.case_equal(emu, content, subsampling, quality)


@pytest.mark.parametrize("i", range(len(J.LARGE)))
def test_large_emu(emu, i):
    J.case_large(emu, i)


@pytest.mark.parametrize("subsampling", J.SUBSAMPLINGS)
def test_ragged_emu(emu, subsampling):
    J.case_ragged(emu, subsampling)


@pytest.mark.parametrize("subsampling", J.SUBSAMPLINGS)
def test_capacity_emu(emu, subsampling):
    J.case_capacity(emu, subsampling)


def test_arguments_emu(emu):
    J.case_arguments(emu)


@pytest.mark.gpu
@pytest.mark.parametrize("content,subsampling,quality", EQUAL)
def test_equal_gpu(gpu, content, subsampling, quality):
    J.case_equal(gpu, content, subsampling, quality)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(J.LARGE)))
def test_large_gpu(gpu, i):
    J.case_large(gpu, i)


@pytest.mark.gpu
@pytest.mark.parametrize("subsampling", J.SUBSAMPLINGS)
def test_ragged_gpu(gpu, subsampling):
    J.case_ragged(gpu, subsampling)


@pytest.mark.gpu
@pytest.mark.parametrize("subsampling", J.SUBSAMPLINGS)
def test_capacity_gpu(gpu, subsampling):
    J.case_capacity(gpu, subsampling)


@pytest.mark.gpu
def test_arguments_gpu(gpu):
    J.case_arguments(gpu)
