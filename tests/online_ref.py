"""Torch-CPU restatement of the online path's loss terms (reference dynaboa_webcam.py), built from the oracle's projection and priors:
the frame term of :233 / :256 / :270 / :301 and cal_motion_loss of :164-182 on the OpenPose BODY_25 window - joints [:, :25] of the
49-joint convention, 25 detections in slots 0..24 of a [B][49][3] keypoint array.  `lo, n` parametrise the window so that the same
code states the gt24 window (25, 24) of base_adaptor.py."""
import torch

from oracle import ref_cpu as O

WINDOWS = {"gt24": (25, 24), "op25": (0, 25)}
KP_CODE = {"gt24": 0, "op25": 1}


def kp2d_loss(pred_s2d, kp, kp_set):
    """(F.mse_loss(pred_s2d[:, window], kp[:, window, :-1], reduction='none') * conf).mean(): the mean runs over B * n * 2."""
    lo, n = WINDOWS[kp_set]
    conf = kp[:, lo:lo + n, 2:3]
    return (((pred_s2d[:, lo:lo + n] - kp[:, lo:lo + n, :2]) ** 2) * conf).mean()


def frame_total(rot, shape, cam, joints, kp, gmm, kp_set, w2d=10.0, wshape=2e-6, wpose=1e-4):
    """-> (s2d, shape prior, pose prior, weighted total) as dynaboa_webcam.py:256-261 forms them."""
    l2d = kp2d_loss(O.projection(cam, joints), kp, kp_set)
    lsh, lpo = O.shape_prior(shape), O.pose_prior(rot, gmm)
    return l2d, lsh, lpo, w2d * l2d + wshape * lsh + wpose * lpo


def motion_loss(cam, joints, h_cam, h_joints, kp, kp_hist, kp_set):
    """cal_motion_loss (:164-182): both projections cut to the window, mask = both frames' confidences are 1."""
    lo, n = WINDOWS[kp_set]
    s2d, h2d = O.projection(cam, joints)[:, lo:lo + n], O.projection(h_cam, h_joints)[:, lo:lo + n]
    pred_motion = s2d - h2d
    gt_motion = kp[:, lo:lo + n, :2] - kp_hist[:, lo:lo + n, :2]
    conf = ((kp_hist[:, lo:lo + n, 2:3] + kp[:, lo:lo + n, 2:3]) == 2).float()
    return (((pred_motion - gt_motion) ** 2) * conf).mean()


def history_rule(n, interval):
    """Frame index n of a stream (0-based): save_hist stores history[n] and THEN increments global_step (:102-105), so the level code
    sees global_step = n + 1.  -> (motion term active, index of the history frame it reads or None): active iff n + 1 - interval > 0,
    reading history[n + 1 - interval] - interval - 1 frames back."""
    gs = n + 1
    on = (gs - interval) > 0
    return on, (gs - interval if on else None)
