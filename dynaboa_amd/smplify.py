"""SMPLify, the optimisation-based fitter of the reference (``utils/smplify/``: ``SMPLify``, ``camera_fitting_loss``,
``body_fitting_loss``, ``gmof``, ``angle_prior``) on the kernels of csrc/smplify.hip.  It refines a predicted pose, shape and camera
against 2-D keypoints: the post-pass for inputs without ground truth.

``SMPLify(native=True)`` runs the whole of ``SMPLify.__call__`` (2 x num_iters Adam iterations and the final forward) in one library
call, dyb_smplify_fit; ``native=False`` runs the reference's control flow as an autograd composition - the ``SMPL`` module (whose
axis-angle input is differentiable through dyb_rodrigues_bwd), the two loss functions below and ``torch.optim.Adam`` on device
tensors - the A/B and a second implementation to cross-check.

One deviation from the reference: it zeroes the confidences of the five ignored joints IN the caller's ``keypoints_2d`` (it writes
into a view, smplify.py:108, :159).  Here the caller's tensor is never written; the mask is applied inside."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib, constants as C
from ._abi import check
from .hmr import stream_of

IGN_JOINTS = ("OP Neck", "OP RHip", "OP LHip", "Right Hip", "Left Hip")         # smplify.py:31
IGN_JOINT_IDS = tuple(C.JOINT_NAMES.index(n) for n in IGN_JOINTS)
CROP_FOCAL, CROP_RES = C.FOCAL_LENGTH, float(C.IMG_RES)


# Body-pose (no global orientation) components that bend the elbows (joints 18, 19: y) and the knees (joints 4, 5: x), and the sign
# of the bend that is natural for each; the body loss kernel carries the same four (csrc/smplify.hip).
BEND_IDS = (52, 55, 9, 12)
BEND_SIGNS = (1.0, -1.0, -1.0, -1.0)


def gmof(x, sigma):
    """The Geman-McClure robust error s2 x2 / (s2 + x2): x2 for |x| << sigma, saturating at s2."""
    s2 = sigma * sigma
    d2 = x * x
    return s2 * d2 / (s2 + d2)


def angle_prior(pose):
    """(B, 4) penalty exp(+-angle)^2 on the elbow and knee bends of the (B, 69) body pose: it grows when one bends the wrong way."""
    bend = pose[:, list(BEND_IDS)] * pose.new_tensor(BEND_SIGNS)
    return torch.exp(bend).square()


def _f32(t):
    return t.detach().contiguous().float()


def _kp(joints_2d, joints_conf):
    return torch.cat([joints_2d.detach().float(), joints_conf.detach().float().unsqueeze(-1)], -1).contiguous()


class _CameraLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, joints, cam_t, cam_t_est, center, kp, focal, depth_w):
        B, dev = joints.shape[0], joints.device
        joints, cam_t, cam_t_est, center = _f32(joints), _f32(cam_t), _f32(cam_t_est), _f32(center)     # locals: alive over the call
        loss = torch.empty(B, device=dev)
        dj, dc = torch.empty(B, 49, 3, device=dev), torch.empty(B, 3, device=dev)
        check(_lib.load().dyb_smplify_camera_loss(joints.data_ptr(), cam_t.data_ptr(), cam_t_est.data_ptr(), center.data_ptr(),
                                                  kp.data_ptr(), float(focal), float(depth_w), loss.data_ptr(), dj.data_ptr(), dc.data_ptr(),
                                                  B, stream_of(joints)), "dyb_smplify_camera_loss")
        ctx.save_for_backward(dj, dc)
        return loss

    @staticmethod
    def backward(ctx, g):
        dj, dc = ctx.saved_tensors
        return dj * g.reshape(-1, 1, 1), dc * g.reshape(-1, 1), None, None, None, None, None


def camera_fitting_loss(model_joints, camera_t, camera_t_est, camera_center, joints_2d, joints_conf, focal_length=5000,
                        depth_loss_weight=100):
    """Stage 1's objective (the reference's losses.py:83-113), summed over the batch: squared reprojection error at the four torso
    joints (the OpenPose ones where all four were detected, else the ground-truth-style ones; chosen per sample) plus the squared,
    weighted distance of the depth from its estimate.  Differentiable in the joints and the camera translation.  One launch: value
    and gradient."""
    return _CameraLoss.apply(model_joints, camera_t, camera_t_est, camera_center, _kp(joints_2d, joints_conf), focal_length,
                             depth_loss_weight).sum()


class _BodyLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, body_pose, betas, joints, cam_t, center, kp, prior, focal, sigma, w_pose, w_shape, w_angle, ignore):
        B, dev = joints.shape[0], joints.device
        body_pose, betas, joints, cam_t = _f32(body_pose).reshape(B, 69), _f32(betas), _f32(joints), _f32(cam_t)
        center = _f32(center)
        f = lambda *s: torch.empty(*s, device=dev)
        parts, reproj, dj, dp, db, dc = f(B, 5), f(B, 49), f(B, 49, 3), f(B, 69), f(B, 10), f(B, 3)
        check(_lib.load().dyb_smplify_body_loss(body_pose.data_ptr(), 69, betas.data_ptr(), 10, joints.data_ptr(), cam_t.data_ptr(),
                                                center.data_ptr(), kp.data_ptr(), prior.means.data_ptr(), prior.precisions.data_ptr(),
                                                prior.log_nll_weights.data_ptr(), float(focal), float(sigma), float(w_pose), float(w_shape),
                                                float(w_angle), int(ignore), parts.data_ptr(), reproj.data_ptr(), None, dj.data_ptr(),
                                                dp.data_ptr(), 69, db.data_ptr(), 10, dc.data_ptr(), B, stream_of(joints)),
              "dyb_smplify_body_loss")
        ctx.save_for_backward(dp, db, dj, dc)
        ctx.mark_non_differentiable(reproj, parts)
        return parts[:, 4].clone(), reproj, parts

    @staticmethod
    def backward(ctx, g, _gr, _gp):
        dp, db, dj, dc = ctx.saved_tensors
        g1 = g.reshape(-1, 1)
        return (dp * g1, db * g1, dj * g.reshape(-1, 1, 1), dc * g1) + (None,) * 9


def body_fitting_loss(body_pose, betas, model_joints, camera_t, camera_center, joints_2d, joints_conf, pose_prior, focal_length=5000,
                      sigma=100, pose_prior_weight=4.78, shape_prior_weight=5, angle_prior_weight=15.2, output='sum', ignore_joints=False):
    """Stage 2's objective (the reference's losses.py:49-81): confidence-weighted GMoF reprojection terms, the mixture pose prior,
    the elbow / knee bend prior and the shape regulariser, in one launch with their gradients.  output='sum': the total summed over the batch, differentiable in the body
    pose, the betas, the joints and the camera translation; output='reprojection': the (B, 49) confidence-weighted robust
    reprojection terms (a value: not differentiable).  ``ignore_joints`` (not in the reference) counts the five joints of
    smplify.py:31 with confidence 0 without touching ``joints_conf``.  ``pose_prior`` is a dynaboa_amd.losses.MaxMixturePrior."""
    total, reproj, _parts = _BodyLoss.apply(body_pose, betas, model_joints, camera_t, camera_center, _kp(joints_2d, joints_conf), pose_prior,
                                            focal_length, sigma, pose_prior_weight, shape_prior_weight, angle_prior_weight, ignore_joints)
    if output == 'sum':
        return total.sum()
    if output == 'reprojection':
        return reproj
    raise ValueError(f"output {output!r}: 'sum' or 'reprojection'")


def crop_cam_to_cam_t(cam):
    """Weak-perspective crop camera (s, tx, ty) -> translation [tx, ty, 2 * 5000 / (224 s + 1e-9)] (base_adaptor.py:160-170)."""
    return torch.stack([cam[:, 1], cam[:, 2], 2 * CROP_FOCAL / (CROP_RES * cam[:, 0] + 1e-9)], -1)


def cam_t_to_crop_cam(cam_t):
    """The inverse of crop_cam_to_cam_t: translation -> (s, tx, ty)."""
    return torch.stack([(2 * CROP_FOCAL / cam_t[:, 2] - 1e-9) / CROP_RES, cam_t[:, 0], cam_t[:, 1]], -1)


def crop_kp_to_pixels(kp2d):
    """(B, 49, 3) keypoints with [-1, 1] crop coordinates -> 224-pixel coordinates about the centre 112 (confidence kept)."""
    return torch.cat([kp2d[..., :2] * (CROP_RES / 2) + CROP_RES / 2, kp2d[..., 2:]], -1)


class SMPLify:
    """The two-stage keypoint fitter behind the reference's ``SMPLify`` name and constructor arguments (its smplify.py:16-175), plus
    ``smpl`` (a dynaboa_amd.smpl.SMPL; required - no model files are read here), ``prior`` (a losses.MaxMixturePrior; default: the
    shipped float32 tables) and ``native`` (module docstring).  ``smpl`` and ``prior`` are modules and ``.to(device)`` moves a module
    in place: the caller's objects end up on ``device``, they are not copied.  ``last_losses`` holds the (2 * num_iters, B) per-sample
    loss of every iteration of the last call, each evaluated before its step."""

    def __init__(self, step_size=1e-2, batch_size=66, num_iters=100, focal_length=5000, device=torch.device('cuda'), smpl=None,
                 prior=None, native=True):
        from .losses import MaxMixturePrior
        if smpl is None:
            raise ValueError("SMPLify needs smpl=: a dynaboa_amd.smpl.SMPL (e.g. BaseAdaptor.smpl_neutral)")
        self.device = torch.device(device)
        self.focal_length, self.step_size, self.num_iters, self.native = focal_length, step_size, num_iters, bool(native)
        self.batch_size = batch_size
        self.ign_joints = list(IGN_JOINT_IDS)
        self.pose_prior = (prior if prior is not None else MaxMixturePrior()).to(self.device)
        self.smpl = smpl.to(self.device)
        self.last_losses = None
        self._ws = None

    # ---------------------------------------------------------------------------------------------------------- native
    def _fit_native(self, init_pose, init_betas, init_cam_t, camera_center, keypoints_2d, num_iters, focal):
        lib = _lib.load()
        B, dev = init_pose.shape[0], init_pose.device
        f = lambda *s: torch.empty(*s, device=dev)
        verts, joints, pose, betas, cam_t, reproj = f(B, C.NUM_VERTS, 3), f(B, 49, 3), f(B, 72), f(B, 10), f(B, 3), f(B, 49)
        log = f(2 * num_iters, B) if num_iters else None
        wsb = int(lib.dyb_smplify_fit_workspace_bytes(B))
        if self._ws is None or self._ws.numel() < wsb or self._ws.device != dev:
            self._ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        p = self.pose_prior
        pose0, betas0, cam0, center, kp = (_f32(t) for t in (init_pose, init_betas, init_cam_t, camera_center, keypoints_2d))
        check(lib.dyb_smplify_fit(self.smpl._pf, self.smpl._pi, p.means.data_ptr(), p.precisions.data_ptr(), p.log_nll_weights.data_ptr(),
                                  pose0.data_ptr(), betas0.data_ptr(), cam0.data_ptr(), center.data_ptr(), kp.data_ptr(), int(num_iters),
                                  float(self.step_size), float(focal), verts.data_ptr(), joints.data_ptr(), pose.data_ptr(),
                                  betas.data_ptr(), cam_t.data_ptr(), reproj.data_ptr(), None if log is None else log.data_ptr(), B,
                                  self._ws.data_ptr(), wsb, stream_of(init_pose)), "dyb_smplify_fit")
        self.last_losses = log
        return verts, joints, pose, betas, cam_t, reproj

    # ----------------------------------------------------------------------------------------------------- composition
    def _fit_autograd(self, init_pose, init_betas, init_cam_t, camera_center, keypoints_2d, num_iters, focal):
        """The same fit as dyb_smplify_fit, held together by autograd: one routine runs both stages, which differ in the leaves
        they move and in the loss head."""
        leaf = lambda t: t.detach().float().clone()
        orient, body, shape, cam = leaf(init_pose[:, :3]), leaf(init_pose[:, 3:]), leaf(init_betas), leaf(init_cam_t)
        kp = _kp(keypoints_2d[..., :2], keypoints_2d[..., -1])            # a packed copy: the caller's tensor is only read
        log = []

        def forward():
            return self.smpl(global_orient=orient, body_pose=body, betas=shape)

        def camera_head(joints):                                          # per-sample values; depth weight: the loss's default
            return _CameraLoss.apply(joints, cam, init_cam_t, camera_center, kp, focal, 100)

        def body_head(joints):                                            # the loss's default weights, the five joints masked inside
            return _BodyLoss.apply(body, shape, joints, cam, camera_center, kp, self.pose_prior, focal, 100, 4.78, 5, 15.2, True)

        def stage(leaves, per_sample):
            """num_iters steps of a fresh Adam (zero moments; torch's default moments 0.9 / 0.999 and eps 1e-8 are the fitter's) over
            ``leaves``.  The batch loss is the sum over samples, so every sample descends its own loss."""
            for t in leaves:
                t.requires_grad_(True)
            opt = torch.optim.Adam(leaves, lr=self.step_size)
            for _ in range(num_iters):
                values = per_sample(forward().joints)
                log.append(values.detach())
                opt.zero_grad()
                values.sum().backward()
                opt.step()
            for t in leaves:
                t.requires_grad_(False)

        stage([orient, cam], camera_head)                                 # stage 1: where the body stands and which way it faces
        stage([orient, body, shape], lambda j: body_head(j)[0])           # stage 2: the body itself, camera fixed
        with torch.no_grad():
            out = forward()
            reproj = body_head(out.joints)[1]
        self.last_losses = torch.stack(log) if log else None
        return out.vertices, out.joints, torch.cat([orient, body], -1), shape, cam, reproj

    def _fit(self, init_pose, init_betas, init_cam_t, camera_center, keypoints_2d, num_iters, focal):
        run = self._fit_native if self.native else self._fit_autograd
        return run(init_pose, init_betas, init_cam_t, camera_center, keypoints_2d, num_iters, focal)

    def __call__(self, init_pose, init_betas, init_cam_t, camera_center, keypoints_2d, num_iters: Optional[int] = None):
        """Fit a batch.  init_pose (B, 72) axis-angle, init_betas (B, 10), init_cam_t (B, 3), camera_center (B, 2), keypoints_2d
        (B, 49, 3) pixels and confidence (left unchanged) -> (vertices, joints, pose, betas, camera_translation,
        reprojection_loss (B, 49)).  ``num_iters`` overrides the constructor's count for this call."""
        n = self.num_iters if num_iters is None else num_iters
        return self._fit(init_pose, init_betas, init_cam_t, camera_center, keypoints_2d, n, self.focal_length)

    def get_fitting_loss(self, pose, betas, cam_t, camera_center, keypoints_2d):
        """The (B, 49) reprojection terms of a given pose, shape and camera, the five joints ignored: what a fit returns last
        (the reference's smplify.py:141-175; ``keypoints_2d`` is left unchanged here too)."""
        with torch.no_grad():
            out = self.smpl(global_orient=pose[:, :3], body_pose=pose[:, 3:], betas=betas)
            return body_fitting_loss(pose[:, 3:], betas, out.joints, cam_t, camera_center, keypoints_2d[:, :, :2], keypoints_2d[:, :, -1],
                                     self.pose_prior, focal_length=self.focal_length, output='reprojection', ignore_joints=True)

    # ------------------------------------------------------------------------------------------------------ crop bridge
    def refine(self, rotmat, betas, cam, kp2d):
        """From this project's outputs: rotmat (B, 24, 3, 3), betas (B, 10), the weak-perspective crop camera (B, 3) and keypoints
        (B, 49, 3) in [-1, 1] crop coordinates -> the fitted result as a dict: ``vts``, ``s3d``, ``rotmat``, ``shape``, ``cam`` (crop
        camera again), ``pose`` (axis-angle), ``cam_t``, ``reprojection_loss``.  Runs at the crop's own focal length and centre."""
        from .smpl import _rodrigues_fwd
        B, dev = rotmat.shape[0], rotmat.device
        R = _f32(rotmat).reshape(B * 24, 3, 3)
        aa = torch.empty(B * 24, 3, device=dev)
        check(_lib.load().dyb_rotmat_to_aa_fwd(R.data_ptr(), aa.data_ptr(), B * 24, stream_of(R)), "dyb_rotmat_to_aa_fwd")
        center = torch.full((B, 2), CROP_RES / 2, device=dev)
        vts, s3d, pose, shape, cam_t, reproj = self._fit(aa.view(B, 72), betas, crop_cam_to_cam_t(_f32(cam)), center,
                                                         crop_kp_to_pixels(_f32(kp2d)), self.num_iters, CROP_FOCAL)
        return {"vts": vts, "s3d": s3d, "rotmat": _rodrigues_fwd(pose.reshape(-1, 3).contiguous()).view(B, 24, 3, 3), "shape": shape,
                "cam": cam_t_to_crop_cam(cam_t), "pose": pose, "cam_t": cam_t, "reprojection_loss": reproj}
