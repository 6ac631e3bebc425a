"""The reference's metric surface (utils/pose_utils.py): Procrustes alignment for PA-MPJPE (:9-64), PCK / AUC (:66-114) and the
acceleration error (:116-144).

``pa_mpjpe_device`` and ``sequence_metrics_device`` are what the adaptation drivers use: the alignment, the errors and the
per-sequence means run in libdynaboa_hip.so (csrc/losses.hip, csrc/seq_metrics.hip; one 3x3 SVD per sample) so the metric path
ships scalars.  The NumPy functions keep the reference's signatures and return conventions (they are also the checkers of the
kernels' tests)."""
from __future__ import annotations

import numpy as np
import torch


def pa_mpjpe_device(pred: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """pred, gt: (n, J, 3) device tensors -> (n,) Procrustes-aligned mean per-joint error, same unit."""
    from . import _lib
    from ._abi import check
    from .hmr import stream_of
    pred, gt = pred.contiguous().float(), gt.contiguous().float()
    n, J = pred.shape[0], pred.shape[1]
    out = torch.empty(n, dtype=torch.float32, device=pred.device)
    check(_lib.load().dyb_pa_mpjpe(pred.data_ptr(), gt.data_ptr(), out.data_ptr(), None, n, J, stream_of(pred)), "dyb_pa_mpjpe")
    return out


def compute_similarity_transform_batch(S1: np.ndarray, S2: np.ndarray) -> np.ndarray:
    """Similarity-align every S1[i] (N,3) onto S2[i]; returns the aligned copies."""
    S1 = np.asarray(S1, np.float32)
    S2 = np.asarray(S2, np.float32)
    mu1, mu2 = S1.mean(1, keepdims=True), S2.mean(1, keepdims=True)
    X1, X2 = S1 - mu1, S2 - mu2
    var1 = (X1 ** 2).sum((1, 2))
    K = np.einsum("bni,bnj->bij", X1, X2)                    # 3x3 = X1^T X2 per sample
    U, s, Vh = np.linalg.svd(K)
    V = np.swapaxes(Vh, 1, 2)
    Z = np.tile(np.eye(3, dtype=S1.dtype), (S1.shape[0], 1, 1))
    Z[:, 2, 2] = np.sign(np.linalg.det(U @ Vh))
    R = V @ Z @ np.swapaxes(U, 1, 2)
    scale = np.einsum("bij,bji->b", R, K) / var1
    t = mu2 - scale[:, None, None] * (mu1 @ np.swapaxes(R, 1, 2))
    return scale[:, None, None] * (S1 @ np.swapaxes(R, 1, 2)) + t


def compute_similarity_transform(S1: np.ndarray, S2: np.ndarray) -> np.ndarray:
    """Reference :9-57 for one sample, in the inputs' precision: the similarity transform (s R, t) that takes S1 (3 x N, or N x 3,
    transposed on the way in and out as the reference does) closest to S2; returns the aligned S1."""
    S1, S2 = np.asarray(S1), np.asarray(S2)
    transposed = False
    if S1.shape[0] != 3 and S1.shape[0] != 2:
        S1, S2, transposed = S1.T, S2.T, True
    assert S2.shape[1] == S1.shape[1]
    mu1, mu2 = S1.mean(axis=1, keepdims=True), S2.mean(axis=1, keepdims=True)
    X1, X2 = S1 - mu1, S2 - mu2
    var1 = np.sum(X1 ** 2)
    K = X1.dot(X2.T)
    U, s, Vh = np.linalg.svd(K)
    V = Vh.T
    Z = np.eye(U.shape[0])
    Z[-1, -1] *= np.sign(np.linalg.det(U.dot(V.T)))
    R = V.dot(Z.dot(U.T))
    scale = np.trace(R.dot(K)) / var1
    t = mu2 - scale * (R.dot(mu1))
    S1_hat = scale * R.dot(S1) + t
    return S1_hat.T if transposed else S1_hat


def compute_pck(s1, s2, threshold) -> np.ndarray:
    """Per sample, the fraction of joints closer than `threshold` (strict <), on the pair as given (reference :66-73).  The
    reference re-stacks its list inside its loop and raises AttributeError from the second sample on; this returns the per-sample
    array for any count and equals the reference on one sample."""
    return np.array([np.mean(np.linalg.norm(np.asarray(kp1) - np.asarray(kp2), axis=1) < threshold) for kp1, kp2 in zip(s1, s2)])


def reconstruction_error(S1, S2, alpha=0.15, needpck=False, needauc=False, reduction='mean'):
    """Reference :76-114: the Procrustes-aligned mean per-joint error per sample (reduced by 'mean' / 'sum', or left per sample) and,
    on request, PCK at 0.15 and the AUC over np.linspace(0, 150, 31) / 1000 - both on the UNALIGNED pair, as the reference computes
    them (`alpha` is unused there too).  Returns re, (re, pck), (re, auc) or (re, pck, auc)."""
    S1, S2 = np.asarray(S1), np.asarray(S2)
    if needpck:
        pck_150 = compute_pck(S1, S2, threshold=0.15)
    if needauc:
        auc = np.mean([compute_pck(S1, S2, threshold / 1000) for threshold in np.linspace(0, 150, 31)])
    S1_hat = np.zeros_like(S1)
    for i in range(S1.shape[0]):
        S1_hat[i] = compute_similarity_transform(S1[i], S2[i])
    re = np.sqrt(((S1_hat - S2) ** 2).sum(axis=-1)).mean(axis=-1)
    if reduction == 'mean':
        re = re.mean()
    elif reduction == 'sum':
        re = re.sum()
    if needauc and needpck:
        return re, pck_150, auc
    if needauc:
        return re, auc
    if needpck:
        return re, pck_150
    return re


def compute_error_accel(joints_gt, joints_pred, vis=None) -> np.ndarray:
    """Reference :116-144: per triple of consecutive frames the mean over joints of |accel_pred - accel_gt|, accel = X[i-1] - 2 X[i]
    + X[i+1]; with `vis` (N,) every triple that holds an invisible frame is dropped.  Returns one value per kept triple."""
    joints_gt, joints_pred = np.asarray(joints_gt), np.asarray(joints_pred)
    accel_gt = joints_gt[:-2] - 2 * joints_gt[1:-1] + joints_gt[2:]
    accel_pred = joints_pred[:-2] - 2 * joints_pred[1:-1] + joints_pred[2:]
    normed = np.linalg.norm(accel_pred - accel_gt, axis=2)
    if vis is None:
        new_vis = np.ones(len(normed), dtype=bool)
    else:
        invis = np.logical_not(vis)
        new_vis = np.logical_not(invis[:-2] | invis[1:-1] | invis[2:])
    return np.mean(normed[new_vis], axis=1)


# columns of sequence_metrics_device's outputs (DYB_SEQM_* of include/dynaboa_hip.h)
FRAME_MPJPE, FRAME_PAMPJPE, FRAME_PCK, FRAME_AUC, FRAME_ACCEL, FRAME_ACCEL_COUNTED, FRAME_FLOATS = 0, 1, 2, 3, 4, 5, 6
SEQ_FRAMES, SEQ_MPJPE, SEQ_PAMPJPE, SEQ_PCK, SEQ_AUC, SEQ_ACCEL, SEQ_TRIPLES, SEQ_FLOATS = 0, 1, 2, 3, 4, 5, 6, 7
AUC_THRESHOLDS = np.linspace(0, 150, 31) / 1000                 # reference :87-91


def sequence_metrics_device(pred: torch.Tensor, gt: torch.Tensor, lengths, valid=None, frame_id=None, pck_thr: float = 0.15,
                            thresholds=None):
    """pred, gt: (n, J, 3) device tensors in one unit, the frames of len(lengths) sequences one after the other (lengths: ints
    summing to n, zeros allowed); valid (n,) bool and frame_id (n,) int tensors are optional -> (frame (n, FRAME_FLOATS),
    seq (len(lengths) + 1, SEQ_FLOATS)) device tensors, the columns named above; the last row of seq covers all frames.  One
    dyb_seq_metrics call on pred's stream; nothing is copied to the host."""
    from . import _lib
    from ._abi import check
    from .hmr import stream_of
    pred, gt = pred.contiguous().float(), gt.contiguous().float()
    n, J = int(pred.shape[0]), int(pred.shape[1])
    lengths = [int(v) for v in lengths]
    if not lengths or min(lengths) < 0 or sum(lengths) != n or gt.shape != pred.shape:
        raise ValueError(f"sequence lengths {lengths} do not tile {n} frames")
    dev = pred.device
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int32).to(dev)
    thr = torch.tensor(np.asarray(AUC_THRESHOLDS if thresholds is None else thresholds, np.float64), dtype=torch.float32).to(dev)
    if valid is not None:
        valid = valid.to(dev).reshape(n).to(torch.uint8).contiguous()
    if frame_id is not None:
        frame_id = frame_id.to(dev).reshape(n).to(torch.int32).contiguous()
    frame = torch.empty(n, FRAME_FLOATS, dtype=torch.float32, device=dev)
    seq = torch.empty(len(lengths) + 1, SEQ_FLOATS, dtype=torch.float32, device=dev)
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
    check(_lib.load().dyb_seq_metrics(ptr(pred), ptr(gt), offsets.data_ptr(), len(lengths), ptr(valid), ptr(frame_id), float(pck_thr),
                                      ptr(thr), int(thr.numel()), ptr(frame), seq.data_ptr(), n, J, stream_of(pred)), "dyb_seq_metrics")
    return frame, seq
