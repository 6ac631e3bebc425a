"""The 3DPW extraction on the MI355X: the kernel cases of tests/pw3d_cases.py on the device, and dynaboa_amd.pw3d_extract on cuda:0
against golden g13, through the loader, under its own rules and through the command."""
import pytest

import pw3d_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def be():
    from backends import GpuBackend
    return GpuBackend()


@pytest.mark.parametrize("n", C.NS)
def test_annotate_against_the_restatement(be, n):
    C.case_seeded(be, n)


def test_fp32_rounding_of_the_translated_joint(be):
    C.case_rounding(be)


@pytest.mark.parametrize("sign", [1, -1], ids=["positive", "negative"])
def test_extrema_come_from_the_49_joints_only(be, sign):
    C.case_lanes(be, sign)


def test_annotate_against_the_reference(be):
    C.case_golden_kernel(be)


def test_error_codes(be):
    C.case_error_codes(be)


@pytest.fixture(scope="module")
def smpls():
    return C.smpl_pair(DEV)


@pytest.fixture(scope="module")
def full(smpls, tmp_path_factory):
    return C.extract_g13(DEV, tmp_path_factory.mktemp("g13"), smpls)[1]


def test_annotate_wrapper():
    C.case_annotate_wrapper(DEV)


def test_extract_sequence_against_the_reference(full):
    C.case_extract_golden(full)


def test_round_trip_through_the_loader(full, tmp_path):
    C.case_round_trip(full, tmp_path)


def test_own_rules(smpls, full, tmp_path):
    C.case_own_rules(DEV, tmp_path, smpls, full)


def test_command_with_check(smpls, tmp_path, monkeypatch, capsys):
    C.case_command(DEV, tmp_path, smpls, monkeypatch, capsys)


def test_order(smpls, tmp_path):
    C.case_order(DEV, tmp_path, smpls)
