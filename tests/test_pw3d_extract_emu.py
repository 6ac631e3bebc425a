"""The 3DPW extraction on the CPU: dyb_pw3d_annotate of csrc/pw3d_extract.hip on the host build of the product sources (tests/emu)
against the fp64 restatement and golden g13, and dynaboa_amd.pw3d_extract with that library swapped in (``_lib.use_library``): SMPL
and ``annotate`` then run the host-compiled kernels on CPU tensors, so every module test below runs the real route end to end - only
the command test replaces something, the reader of SMPL_*.pkl files.  tests/pw3d_cases.py states the bounds."""
import pytest

import pw3d_cases as C


@pytest.fixture(scope="module")
def be():
    from backends import EmuBackend
    return EmuBackend()


# ---- the kernel through the C ABI
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


# ---- the module on the host build
@pytest.fixture(scope="module")
def emu_python(be):
    from dynaboa_amd import _lib
    saved = _lib._lib
    _lib.use_library(be.lib)
    yield
    _lib._lib = saved


@pytest.fixture(scope="module")
def smpls(emu_python):
    return C.smpl_pair("cpu")


@pytest.fixture(scope="module")
def full(emu_python, smpls, tmp_path_factory):
    """The g13 sequence extracted once; shared, never rewritten."""
    return C.extract_g13("cpu", tmp_path_factory.mktemp("g13"), smpls)[1]


def test_annotate_wrapper(emu_python):
    C.case_annotate_wrapper("cpu")


def test_extract_sequence_against_the_reference(full):
    C.case_extract_golden(full)


def test_round_trip_through_the_loader(full, tmp_path):
    C.case_round_trip(full, tmp_path)


def test_own_rules(smpls, full, tmp_path):
    C.case_own_rules("cpu", tmp_path, smpls, full)


def test_command_with_check(smpls, tmp_path, monkeypatch, capsys):
    C.case_command("cpu", tmp_path, smpls, monkeypatch, capsys)


def test_order(smpls, tmp_path):
    C.case_order("cpu", tmp_path, smpls)
