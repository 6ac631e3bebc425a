"""dyb_seq_metrics (csrc/seq_metrics.hip) against the reference's outputs (golden g14, tools/make_golden_seq_metrics.py) and the NumPy
surface of dynaboa_amd/pose_utils.py, through the cases of tests/seq_metrics_cases.py: on the kernel emulator and, marked gpu, on the
device through the same C ABI.  The NumPy surface itself is held to the golden here too."""
import numpy as np
import pytest

import seq_metrics_cases as SC
from backends import EmuBackend, GpuBackend
from conftest import golden
from dynaboa_amd import pose_utils as PU


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


@pytest.fixture(scope="module")
def gpu():
    return GpuBackend()


def test_inputs_keep_a_margin_from_every_threshold():
    """No joint distance of the test's own inputs (which are the golden's) lies within MARGIN of the PCK threshold or an AUC
    threshold: no rounding can decide a PCK, which is what lets PCK and AUC be compared to 1e-6."""
    g = golden("g14_seq_metrics.npz")
    assert tuple(g["lengths"]) == SC.LENGTHS
    for J in SC.JOINTS:
        pred, gt = SC.make_batch(J)
        assert np.array_equal(g[f"pred{J}"], pred) and np.array_equal(g[f"gt{J}"], gt)
        assert SC.margin(pred, gt) >= SC.MARGIN


@pytest.mark.parametrize("J", SC.JOINTS)
def test_numpy_surface_equals_the_reference(J):
    """reconstruction_error / compute_pck / compute_error_accel on every stored case of the golden (float64 in, as it was made)."""
    g = golden("g14_seq_metrics.npz")
    p, t = g[f"pred{J}"].astype(np.float64), g[f"gt{J}"].astype(np.float64)
    re, pck, auc = [], [], []
    for i in range(len(p)):
        r = PU.reconstruction_error(p[i:i + 1], t[i:i + 1], needpck=True, needauc=True, reduction=None)
        re.append(r[0][0]); pck.append(r[1][0]); auc.append(r[2])
    assert np.abs(np.array(re) - g[f"re{J}"]).max() <= 1e-12
    assert np.array_equal(np.array(pck), g[f"pck{J}"]) and np.abs(np.array(auc) - g[f"auc{J}"]).max() <= 1e-15
    off = SC.offsets_of(SC.LENGTHS)
    vis = g["vis"].astype(bool)
    for s, n in enumerate(SC.LENGTHS):
        if n >= 3:
            a, b = off[s], off[s + 1]
            assert np.array_equal(PU.compute_error_accel(t[a:b], p[a:b]), g[f"accel{J}_s{s}"])
            assert np.array_equal(PU.compute_error_accel(t[a:b], p[a:b], vis[a:b]), g[f"accel_vis{J}_s{s}"])
    assert len(g[f"accel_vis{J}_s5"]) == 60 and len(g[f"accel{J}_s5"]) == 63


def test_reconstruction_error_return_shapes_and_pck_on_three_samples():
    """The reference's tuple shapes for the four flag combinations; compute_pck on 3 samples (where the reference raises) equals the
    single-sample values."""
    pred, gt = SC.make_batch(14)
    p, t = pred[70:73].astype(np.float64), gt[70:73].astype(np.float64)
    re = PU.reconstruction_error(p, t)
    assert np.ndim(re) == 0
    assert PU.reconstruction_error(p, t, reduction=None).shape == (3,)
    assert PU.reconstruction_error(p, t, reduction='sum') == pytest.approx(3 * re)
    r = PU.reconstruction_error(p, t, needpck=True)
    assert len(r) == 2 and r[0] == re and r[1].shape == (3,)
    r = PU.reconstruction_error(p, t, needauc=True)
    assert len(r) == 2 and r[0] == re and np.ndim(r[1]) == 0
    r = PU.reconstruction_error(p, t, needpck=True, needauc=True)
    assert len(r) == 3 and r[1].shape == (3,) and np.ndim(r[2]) == 0
    pck3 = PU.compute_pck(p, t, 0.15)
    assert pck3.shape == (3,)
    for i in range(3):
        assert pck3[i] == PU.compute_pck(p[i:i + 1], t[i:i + 1], 0.15)[0]
    assert np.array_equal(PU.compute_similarity_transform(p[0], t[0]), PU.compute_similarity_transform(p[0].T, t[0].T).T)


@pytest.mark.parametrize("J", SC.JOINTS)
def test_batch_emu(emu, J):
    SC.case_batch(emu, golden, J)


def test_masks_emu(emu):
    SC.case_masks(emu, golden)


def test_determinism_emu(emu):
    SC.case_determinism(emu)


def test_arguments_emu(emu):
    SC.case_arguments(emu)


@pytest.mark.gpu
@pytest.mark.parametrize("J", SC.JOINTS)
def test_batch_gpu(gpu, J):
    SC.case_batch(gpu, golden, J)


@pytest.mark.gpu
def test_masks_gpu(gpu):
    SC.case_masks(gpu, golden)


@pytest.mark.gpu
def test_determinism_gpu(gpu):
    SC.case_determinism(gpu)


@pytest.mark.gpu
def test_arguments_gpu(gpu):
    SC.case_arguments(gpu)
