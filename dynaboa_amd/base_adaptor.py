"""BaseAdaptor: model / optimiser / teacher set-up, loss assembly for the lower and upper level of
the bilevel adaptation, mean-teacher EMA, frame history and exemplar retrieval.

Mirrors the public surface of reference ``base_adaptor.py::BaseAdaptor`` (lines 36-447): same
constructor argument (the argparse namespace), same method names and return conventions
(``projection`` -> {'ori','normed'}, ``decode_smpl_params`` -> {'s3d','vts'},
``lower/upper_level_adaptation(image, gt_keypoints_2d, h36m_batch, learner)`` -> (loss, features),
``cal_*``), same attributes the drivers read.  What differs is underneath: the model is the native
HIP engine, SMPL / losses / Adam / EMA are HIP kernels, and the frame history stays on the device
instead of round-tripping through NumPy (reference :173-180).

Data that the reference reads from fixed paths (checkpoint, SMPL pickles, regressors, retrieval
clusters) can be injected through ``assets_bundle`` so the path runs on synthetic stand-ins
(dynaboa_amd.assets) where the licensed files are absent.
"""
from __future__ import annotations

import logging
import os
import random
from types import SimpleNamespace
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

from . import assets as A
from . import constants
from .hmr import hmr
from .fused_level import clear_last_forward, level_forward
from .losses import (AUX_MAX_BATCH, KP_WINDOWS, MaxMixturePrior, frame_losses, kp_set_refusal, labelled_term, motion_term, pose_prior, projection_normed,
                     teacher_term)
from .maml import MAML
from .optim import Adam, ema_update
from .smpl import SMPL


def synthetic_bundle(seed: int = 22, identity_pose: bool = True, randomize_norm: bool = False, smpl_seed: int = 0,
                     resident_exemplars: bool = False):
    """Everything BaseAdaptor needs, generated from seeds."""
    mp = A.make_smpl_mean_params(identity_pose=identity_pose, seed=3)
    return SimpleNamespace(
        mean_params=mp,
        checkpoint=A.make_synthetic_checkpoint(seed, mp, randomize_norm=randomize_norm),
        smpl_neutral=A.make_synthetic_smpl(smpl_seed), smpl_male=A.make_synthetic_smpl(smpl_seed + 1),
        smpl_female=A.make_synthetic_smpl(smpl_seed + 2),
        exemplars=lambda step, n: A.make_exemplars_pinned(step, n),
        # opt-in: exemplars resident on the device and shared by every sequence of a step; off = every retrieval()
        # uploads its own copy, as the reference does (base_adaptor.py:82-96)
        exemplars_device=(lambda step, n, device: A.make_exemplars_device(step, n, device)) if resident_exemplars else None,
        dataloader=None, gmm_folder=None)


class BaseAdaptor:
    def __init__(self, options, assets_bundle=None, device=None):
        self.options = options
        self.exppath = os.path.join(getattr(options, "expdir", "exps"), getattr(options, "expname", "run"))
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        self.bundle = assets_bundle
        self.seed_everything(options.seed)
        self.options.mixtrain = options.lower_level_mixtrain or options.upper_level_mixtrain
        self.history: Dict[int, dict] = {}
        self.fit_losses: Dict[str, torch.Tensor] = {}
        self.kp2dlosses_lower, self.kp2dlosses_upper = [], {}
        self.global_step = 0
        if options.retrieval:
            self.load_h36_cluster_res()
            if self.bundle is None:
                # the exemplar set retrieval() draws from (reference base_adaptor.py:55)
                from . import datasets as D
                self.h36m_dataset = D.SourceDataset(self.H36M_SAMPLE_FILE,
                                                    img_dir=getattr(options, "h36m_root", None) or D.H36M_ROOT, device=self.device)
                if getattr(options, "exemplar_bank", 0):
                    # --exemplar_bank 1: the whole set preprocessed once and resident on the device (exemplar_bank.py; one bank per
                    # (files, device), shared by the adaptors of a replica group); retrieval() then follows the bank's draw rule
                    from .exemplar_bank import ExemplarBank
                    self.exemplar_bank = ExemplarBank.from_tree(self.H36M_SAMPLE_FILE, self.H36M_CLUSTER_FILE, self.h36m_dataset.img_dir,
                                                                self.device)
                    self._bank_draw, self._bank_last_pick = 0, None
        self.set_model_optim()
        if options.use_meanteacher:
            self.set_teacher()
        self.set_dataloader()
        self.set_criterion()
        self.setup_smpl()

    # ------------------------------------------------------------------ set-up
    def seed_everything(self, seed):
        random.seed(seed)
        np.random.seed(seed)
        torch.manual_seed(seed)

    def _checkpoint(self):
        if self.bundle is not None:
            return self.bundle.checkpoint
        return torch.load(self.options.model_file, map_location="cpu")

    def _mean_params(self):
        return self.bundle.mean_params if self.bundle is not None else "data/smpl_mean_params.npz"

    def set_model_optim(self):
        ck = self._checkpoint()["model"]
        model = hmr(self._mean_params(), seed=0)
        if self.options.use_boa:
            # the reference hard-codes first_order=True (base_adaptor.py:119); `second_order` is this build's switch
            self.model = MAML(model, lr=self.options.fastlr,
                              first_order=not getattr(self.options, "second_order", 0)).to(self.device)
            self.model.load_state_dict(ck, strict=True)
        else:
            self.model = model.to(self.device)
            self.model.load_state_dict({k.replace("module.", ""): v for k, v in ck.items()}, strict=True)
        self.optimizer = Adam(self.model.parameters(), lr=self.options.lr, betas=(self.options.beta1, self.options.beta2))
        if self.options.use_boa and getattr(self.options, "second_order", 0):
            # this optimiser understands a gradient left as (v, H v, lr): one fused "Adam + accumulate" launch for the outer step
            self.model.defer_accumulate = bool(getattr(self.options, "fused_so_adam", 1))
        # precision of the backbone convolutions is a property of the engine plan (one per batch size, shared by every
        # model of the process): set explicitly both ways so that a bf16 run does not leak into a later fp32 one
        from .hmr import get_layout
        want = bool(getattr(self.options, "bf16_mfma", 0))
        for b in {1, int(getattr(self.options, "batch_size", 1)), int(getattr(self.options, "sample_num", 1))}:
            get_layout(b).set_bf16(want)

    def set_teacher(self):
        teacher = hmr(self._mean_params(), seed=0)
        for p in teacher.parameters():
            p.detach_()
        self.teacher = teacher.to(self.device)
        ck = self._checkpoint()["model"]
        self.teacher.load_state_dict({k.replace("module.", ""): v for k, v in ck.items()}, strict=True)
        # The reference never calls teacher.eval() (base_adaptor.py:151-158): its teacher runs with live Dropout in the
        # regressor, so the teacher targets carry p = 0.5 mask noise.  teacher_dropout=1 reproduces that (the masks come from
        # this build's counter-based generator, so runs agree with the reference in distribution, not sample by sample);
        # the default keeps the teacher deterministic (eval), which is what the goldens pin.  Recorded in DESIGN.md.
        if getattr(self.options, "teacher_dropout", 0):
            self.teacher.train()
        else:
            self.teacher.eval()

    def set_dataloader(self):
        """reference base_adaptor.py:130-137: the 3DPW test stream in sequence order, batch_size frames at a time, decoded
        ahead on 8 host threads; crop / resize / normalise on the GPU (datasets.py).  With a synthetic bundle the stream
        is whatever the caller iterates."""
        if self.bundle is not None:
            self.dataloader = self.bundle.dataloader
            return
        from . import datasets as D
        if getattr(self.options, "dataset", "3dpw") == "internet":
            # reference base_adaptor.py:132-134: the rows of every <internet_root>/*.npz as one stream (internet.py)
            from . import internet as I
            ds = I.InternetDataset(self.options, device=self.device)
            self.imgdir = ds.img_dir
            self.dataloader = D.FrameLoader(ds, batch_size=self.options.batch_size, workers=8) if len(ds) else None
            return
        self.imgdir = getattr(self.options, "pw3d_root", None) or D.PW3D_ROOT
        ds = D.PW3D(self.options, img_dir=self.imgdir, device=self.device)
        self.dataloader = D.FrameLoader(ds, batch_size=self.options.batch_size, workers=8) if len(ds) else None

    def set_criterion(self):
        folder = self.bundle.gmm_folder if self.bundle is not None else "data/spin_data"
        self.gmm_f = MaxMixturePrior(prior_folder=folder, num_gaussians=8).to(self.device)

    def setup_smpl(self):
        if self.bundle is not None:
            self.smpl_neutral = SMPL(tables=self.bundle.smpl_neutral).to(self.device)
            self.smpl_male = SMPL(tables=self.bundle.smpl_male).to(self.device)
            self.smpl_female = SMPL(tables=self.bundle.smpl_female).to(self.device)
            self.J_regressor = torch.from_numpy(self.bundle.smpl_neutral["J_regressor_h36m"]).float()
        else:
            self.smpl_neutral = SMPL("data/smpl", create_transl=False).to(self.device)
            self.smpl_male = SMPL("data/smpl", gender="male", create_transl=False).to(self.device)
            self.smpl_female = SMPL("data/smpl", gender="female", create_transl=False).to(self.device)
            self.J_regressor = torch.from_numpy(np.load("data/J_regressor_h36m.npy")).float()
        self.joint_mapper_h36m = list(constants.H36M_TO_J14)
        self.joint_mapper_gt = list(constants.J24_TO_J14)

    # ------------------------------------------------------------------ retrieval (base_adaptor.py:74-96)
    H36M_SAMPLE_FILE = 'data/retrieval_res/h36m_random_sample_center_10_10.pt'                       # reference base_adaptor.py:55
    H36M_CLUSTER_FILE = "data/retrieval_res/cluster_res_random_sample_center_10_10_potocol2.pt"      # reference base_adaptor.py:76

    def load_h36_cluster_res(self):
        """reference base_adaptor.py:74-80: cluster centres of the base model's Human3.6M features + member indices."""
        self.centers = None
        if self.bundle is None:
            import joblib
            res = self.h36m_cluster_res = joblib.load(self.H36M_CLUSTER_FILE)
            self.centers = torch.from_numpy(np.asarray(res["centers"])).float().to(self.device)
            self.index = res["index"]

    # the exemplars the latest level used: a plain attribute on the autograd and callback routes; with the bank on the device the stepper
    # leaves a recipe (its latest logged pick) and the dict is built when somebody reads it
    @property
    def _last_h36m(self):
        make = self.__dict__.pop("_last_h36m_make", None)
        if make is not None:
            self.__dict__["_last_h36m_value"] = make()
        return self.__dict__.get("_last_h36m_value")

    @_last_h36m.setter
    def _last_h36m(self, batch):
        self.__dict__.pop("_last_h36m_make", None)
        self.__dict__["_last_h36m_value"] = batch

    def defer_last_h36m(self, make):
        self.__dict__["_last_h36m_make"] = make

    def get_h36m_data(self, indice):
        return dict(self.h36m_dataset[indice])

    def retrieval(self, feature):
        """reference base_adaptor.py:82-96: nearest cluster by cosine distance of features[5] (the pooled 2048-vector) to
        the centres, `sample_num` members drawn with the seeded `random` module, their items concatenated along dim 0.
        The cluster index is the one host synchronisation of the level (the reference's `.item()`).
        With --exemplar_bank 1 (no bundle) the nearest centre (ties: lowest index) and the member come from the bank's kernels: draw
        number `_bank_draw` of this adaptor under seed options.seed (exemplar_bank.py) - the rule the native stepper applies on the
        device, so the autograd path, the callback route and the device route pick the same exemplars."""
        bank = getattr(self, "exemplar_bank", None)
        if bank is not None and self.bundle is None:
            if self.options.sample_num != 1:
                raise ValueError("--exemplar_bank 1 draws one exemplar per retrieval (sample_num 1)")
            batch, picks = bank.select(feature, [self._bank_draw], self.options.seed)
            self._bank_draw += 1
            self._bank_last_pick = picks[0]
            return batch
        if self.bundle is not None:
            dev_fn = getattr(self.bundle, "exemplars_device", None)
            if dev_fn is not None:            # synthetic exemplars: resident on the device, one generation per step for all sequences
                return dev_fn(self.global_step, self.options.sample_num, self.device)
            batch = self.bundle.exemplars(self.global_step, self.options.sample_num)
        else:
            dists = 1 - F.cosine_similarity(feature, self.centers)
            pos_cluster = torch.argsort(dists)[0].item()
            pos_indices = random.sample(self.index[pos_cluster], self.options.sample_num)
            items = [self.get_h36m_data(i) for i in pos_indices]
            batch = items[0]
            for it in items[1:]:
                for k, v in it.items():
                    batch[k] = torch.cat([batch[k], v], dim=0) if torch.is_tensor(v) else batch[k]
        return {k: (v.to(self.device, non_blocking=True) if torch.is_tensor(v) else v) for k, v in batch.items()}

    # ------------------------------------------------------------------ geometry helpers
    def projection(self, cam, s3d, eps=1e-9):
        normed = projection_normed(cam, s3d)
        return {"ori": normed * (constants.IMG_RES / 2.0), "normed": normed}

    def decode_smpl_params(self, poses, beta, gender="neutral", pose2rot=False):
        smpl = {"neutral": self.smpl_neutral, "male": self.smpl_male, "female": self.smpl_female}[gender]
        out = smpl(betas=beta, body_pose=poses[:, 1:], global_orient=poses[:, 0].unsqueeze(1), pose2rot=pose2rot)
        return {"s3d": out.joints, "vts": out.vertices}

    # ------------------------------------------------------------------ history (device resident)
    def save_hist(self, image, s2d):
        self.history[self.global_step] = {"image": image.detach(), "s2d": s2d.detach()}
        stale = self.global_step - self.options.interval - 1
        self.history.pop(stale, None)            # the reference never prunes (602 KB/frame host growth)

    def motion_on(self) -> bool:
        """The motion term's gate: a frame `interval` steps back exists (global_step counts from 1 here: save_hist came first)."""
        return bool(self.options.use_motion and (self.global_step - self.options.interval) > 0)

    def get_hist(self):
        h = self.history[self.global_step - self.options.interval]
        return h["image"], h["s2d"]

    # ------------------------------------------------------------------ teacher
    def update_teacher(self, teacher, model):
        ema_update(teacher.parameters(), model.parameters(), self.options.alpha)

    def cal_feature_diff(self, features_i, features_j):
        sims, mean = {}, 0
        for i, (a, b) in enumerate(zip(features_i, features_j)):
            c = F.cosine_similarity(a.flatten(), b.flatten(), dim=0, eps=1e-12)
            mean = mean + c
            sims[i] = {"cos": c}
        self.fit_losses["feat_sim/cos_sim"] = mean / i
        return sims

    # ------------------------------------------------------------------ losses
    def cal_shape_prior(self, pred_betas):
        return (pred_betas ** 2).sum(dim=-1).mean()

    def cal_pose_prior(self, pred_rotmat, betas=None):
        return pose_prior(pred_rotmat, self.gmm_f)

    def cal_s3d_loss(self, pred_s3d, gt_s3d, conf):
        gt = gt_s3d - ((gt_s3d[:, 2] + gt_s3d[:, 3]) / 2)[:, None, :]
        pr = pred_s3d - ((pred_s3d[:, 2] + pred_s3d[:, 3]) / 2)[:, None, :]
        return (conf * (pr - gt) ** 2).mean()

    def cal_teacher_loss(self, image, pred_rotmat, pred_shape, pred_s2d, pred_s3d):
        with torch.no_grad():
            t_rot, t_shape, t_cam = self.teacher(image)
            t_s3d = self.decode_smpl_params(t_rot, t_shape)["s3d"]
            t_s2d = self.projection(t_cam, t_s3d)["normed"]
        terms = dict(s2dloss=F.mse_loss(pred_s2d, t_s2d), s3dloss=F.mse_loss(t_s3d, pred_s3d),
                     shape_loss=F.mse_loss(pred_shape, t_shape), pose_loss=F.mse_loss(pred_rotmat, t_rot))
        loss = terms["s2dloss"] * 5 + terms["s3dloss"] * 5 + terms["shape_loss"] * 0.001 + terms["pose_loss"] * 1
        for k, v in terms.items():
            self.fit_losses[f"teacher/{k}"] = v
        self.fit_losses["teacher/loss"] = loss
        return loss

    def cal_motion_loss(self, model, pred_s2d, gt_s2d, prefix="ul"):
        hist_image, hist_s2d = self.get_hist()
        h_rot, h_shape, h_cam = model(hist_image)
        h_s3d = self.decode_smpl_params(h_rot, h_shape)["s3d"]
        h_s2d = self.projection(h_cam, h_s3d)["normed"]
        lo, n = KP_WINDOWS[getattr(self.options, "kp_set", "gt24")]          # (pred_s2d / gt_s2d arrive cut to the same window)
        pred_motion = pred_s2d - h_s2d[:, lo:lo + n]
        gt_motion = gt_s2d[:, :, :-1] - hist_s2d[:, lo:lo + n, :-1]
        conf = ((hist_s2d[:, lo:lo + n, -1:] + gt_s2d[:, :, -1:]) == 2).float()
        loss = (((pred_motion - gt_motion) ** 2) * conf).mean()
        self.fit_losses[f"{prefix}/motion_loss"] = loss
        return loss

    def _teacher_term(self, image, rot, shape, cam, s3d):
        """cal_teacher_loss on the term kernel (same logging keys)."""
        with torch.no_grad():
            t_rot, t_shape, t_cam = self.teacher(image)
            t_s3d = self.decode_smpl_params(t_rot, t_shape)["s3d"]
        loss, comps = teacher_term(rot, shape, cam, s3d, t_rot, t_shape, t_cam, t_s3d)
        for i, k in enumerate(("s2dloss", "s3dloss", "shape_loss", "pose_loss")):
            self.fit_losses[f"teacher/{k}"] = comps[i]
        self.fit_losses["teacher/loss"] = loss
        return loss

    def _motion_term(self, model, rot, shape, cam, s3d, gt_keypoints_2d, prefix="ul"):
        """cal_motion_loss on the term kernel: the history frame through the same weights, both passes differentiable."""
        hist_image, hist_s2d = self.get_hist()
        h_rot, h_shape, h_cam = model(hist_image)
        h_s3d = self.decode_smpl_params(h_rot, h_shape)["s3d"]
        loss, _ = motion_term(rot, shape, cam, s3d, h_cam, h_s3d, gt_keypoints_2d, hist_s2d, kp_set=getattr(self.options, "kp_set", "gt24"))
        self.fit_losses[f"{prefix}/motion_loss"] = loss
        return loss

    def adapt_on_labeled_data(self, model, batch, prefix="ll", kernels=False):
        from .geometry import batch_rodrigues
        gt_s2d = batch["keypoints"]
        conf = gt_s2d[:, 25:, -1:].clone()
        rot, shape, cam, feats = model(batch["img"], need_feature=True)
        s3d = self.decode_smpl_params(rot, shape)["s3d"]
        gt_rot = batch_rodrigues(batch["pose"].view(-1, 3)).view(-1, 24, 3, 3)
        assert batch["pose_3d"].shape[1] == 24
        if kernels:
            loss, comps = labelled_term(rot, shape, cam, s3d, gt_s2d, gt_rot, batch["betas"], batch["pose_3d"])
            terms = dict(labled_s2dloss=comps[0], labled_s3dloss=comps[1], labled_shape_loss=comps[2], labled_pose_loss=comps[3])
        else:
            s2d = self.projection(cam, s3d)["normed"]
            terms = dict(labled_s2dloss=(((s2d[:, 25:] - gt_s2d[:, 25:, :-1]) ** 2) * conf).mean(),
                         labled_s3dloss=self.cal_s3d_loss(s3d[:, 25:], batch["pose_3d"][:, :, :-1], conf),
                         labled_shape_loss=F.mse_loss(shape, batch["betas"]), labled_pose_loss=F.mse_loss(rot, gt_rot))
            loss = (terms["labled_s2dloss"] * 5 + terms["labled_s3dloss"] * 5 + terms["labled_shape_loss"] * 0.001
                    + terms["labled_pose_loss"] * 1)
        for k, v in terms.items():
            self.fit_losses[f"{prefix}/{k}"] = v
        self.fit_losses[f"{prefix}/labled_loss"] = loss
        return loss, feats

    def _level(self, level, image, gt_keypoints_2d, h36m_batch, learner):
        o = self.options
        tag = "ll" if level == "lower" else "ul"
        kp_set = getattr(o, "kp_set", "gt24")
        why = kp_set_refusal(o)
        if why:
            raise ValueError(why)
        kp_lo, kp_n = KP_WINDOWS[kp_set]
        quiet = getattr(self, "_replay", None) is not None     # a second-order re-evaluation: no logging, same exemplars
        loss = None
        s2d = None
        log = {} if quiet else self.fit_losses
        fused = getattr(o, "fused_level", 1) and getattr(o, f"use_frame_losses_{level}")
        if fused:
            # model -> SMPL -> frame-loss head as ONE autograd node (fused_level.py); same numbers as the
            # three-module composition below, which stays for use_frame_losses_* = 0 and as the cross-check
            loss, comps, rot, shape, cam, s3d, _vts, feats = level_forward(
                learner, self.smpl_neutral, self.gmm_f, image, gt_keypoints_2d, o.s2dloss_weight, o.shape_prior_weight,
                o.pose_prior_weight, kp_set=kp_set)
        else:
            clear_last_forward()                 # (a remembered fused forward must not be mistaken for this level's: ADVICE r3)
            rot, shape, cam, feats = learner(image, need_feature=True)
            smpl_out = self.decode_smpl_params(rot, shape)
            s3d = smpl_out["s3d"]
        if not quiet:
            self._level_pred = (rot.detach(), shape.detach(), cam.detach())     # what inference() with these weights returns
        if getattr(o, f"use_frame_losses_{level}"):
            if not fused:
                loss, comps = frame_losses(rot, shape, cam, s3d, gt_keypoints_2d, self.gmm_f, o.s2dloss_weight,
                                           o.shape_prior_weight, o.pose_prior_weight, kp_set=kp_set)
            if not quiet:
                if level == "lower":
                    self.kp2dlosses_lower.append(comps[0])
                else:
                    self.kp2dlosses_upper[self.global_step] = comps[0]
            log[f"{tag}/s2dloss"], log[f"{tag}/shape_prior"] = comps[0], comps[1]
            log[f"{tag}/pose_prior"], log[f"{tag}/unlabelloss"] = comps[2], loss.detach()
        keep, self.fit_losses = self.fit_losses, log           # the term helpers below log into self.fit_losses
        try:
            # teacher / motion / labelled terms: one value + gradient launch each (losses._AuxTerms) - the same kernel the native
            # stepper issues; --term_kernels 0 (or a batch beyond its 16 samples) composes them from torch ops as the reference does
            kern = bool(getattr(o, "term_kernels", 1)) and image.shape[0] <= AUX_MAX_BATCH
            if getattr(o, f"use_temporal_losses_{level}"):
                if not kern:
                    s2d = self.projection(cam, s3d)["normed"]
                if o.use_meanteacher:
                    t = (self._teacher_term(image, rot, shape, cam, s3d) if kern else self.cal_teacher_loss(image, rot, shape, s2d, s3d))
                    t = t * o.teacherloss_weight
                    loss = t if loss is None else loss + t
                if self.motion_on():
                    m = (self._motion_term(learner, rot, shape, cam, s3d, gt_keypoints_2d, prefix="ul") if kern else
                         self.cal_motion_loss(learner, s2d[:, kp_lo:kp_lo + kp_n], gt_keypoints_2d[:, kp_lo:kp_lo + kp_n], prefix="ul"))
                    loss = loss + m * o.motionloss_weight
            if o.retrieval:
                h36m_batch = self._replay["h36m"] if quiet else self.retrieval(feats[5])
            self._last_h36m = h36m_batch
            if getattr(o, f"{level}_level_mixtrain"):
                lab, _ = self.adapt_on_labeled_data(learner, h36m_batch, prefix=tag,
                                                    kernels=kern and h36m_batch["img"].shape[0] <= AUX_MAX_BATCH)
                loss = loss + lab * o.labelloss_weight
        finally:
            self.fit_losses = keep
        # the reference builds the sum with in-place `loss += ...` on the tensor it stored as
        # '<tag>/unlabelloss' (base_adaptor.py:244,250,254,266), so what it logs under that key is this total
        log[f"{tag}/total"] = loss.detach()
        return loss, feats

    def level_closure(self, level, image, gt_keypoints_2d, h36m_batch):
        """The loss `_level` just returned, as a function of the learner (for MAML.adapt(..., closure=) in
        second-order mode): same data, same retrieved exemplars, nothing logged."""
        used = getattr(self, "_last_h36m", None)

        def closure(learner):
            self._replay = dict(h36m=used)
            try:
                return self._level(level, image, gt_keypoints_2d, h36m_batch, learner)[0]
            finally:
                self._replay = None
        return closure

    def level_hvp_factory(self, level, image, gt_keypoints_2d, learner):
        """With --hvp exact: theta -> (v -> H v) for the level `_level` just evaluated (dynaboa_amd/hvp.py): frame-loss levels
        through the kernels' own head gradient, levels with teacher / motion / labelled terms through the multi-pass form;
        None (MAML.adapt then differences the closure's gradient) with --hvp fd."""
        o = self.options
        if getattr(o, "hvp", "fd") != "exact":
            return None
        from .hvp import frame_level_hvp, general_level_hvp
        hmr = getattr(learner, "module", learner)
        other = getattr(o, f"use_temporal_losses_{level}") or getattr(o, f"{level}_level_mixtrain")
        if not other and getattr(o, f"use_frame_losses_{level}"):
            # frame losses only (the benchmarked second-order configuration): the head's gradient straight from the kernels
            return lambda theta: frame_level_hvp(hmr, self.smpl_neutral, self.gmm_f, theta, image, gt_keypoints_2d, o.s2dloss_weight,
                                                 o.shape_prior_weight, o.pose_prior_weight, head=getattr(o, "hvp_head", "fd"))
        if getattr(o, "hvp_head", "fd") == "closed" and not getattr(self, "_hvp_head_fd_logged", False):
            # teacher / motion / labelled terms have no closed-form second derivative: the whole level keeps the difference quotient of
            # its head (never a mix of the two forms inside one level); said once per run
            self._hvp_head_fd_logged = True
            logging.getLogger(__name__).warning(
                "--hvp_head closed: the %s level has teacher / motion / labelled terms; its head keeps the difference quotient "
                "(--hvp_head fd) - the closed form covers levels made of the frame losses only", level)
        if getattr(o, "hvp_terms", "all") != "all":
            return None                      # --hvp_terms frame: teacher / motion / labelled levels keep the difference quotient
        used = getattr(self, "_last_h36m", None)
        return lambda theta: general_level_hvp(self, level, hmr, theta, image, gt_keypoints_2d, used)

    def lower_level_adaptation(self, image, gt_keypoints_2d, h36m_batch, learner=None):
        return self._level("lower", image, gt_keypoints_2d, h36m_batch, learner)

    def upper_level_adaptation(self, image, gt_keypoints_2d, h36m_batch, learner=None):
        return self._level("upper", image, gt_keypoints_2d, h36m_batch, learner)

    # ------------------------------------------------------------------ stubs the drivers override
    def excute(self):
        pass

    def adaptation(self, batch):
        pass

    def inference(self, batch, model, need_feature=False):
        pass

    # ------------------------------------------------------------------ rendered results (--save_res 1)
    RESULT_COLOR = (205 / 255.0, 129 / 255.0, 98 / 255.0)          # reference base_adaptor.py:442

    def _renderer(self, width, height):
        from .render import Renderer
        cache = self.__dict__.setdefault("_renderers", {})
        key = (int(width), int(height))
        if key not in cache:
            cache.clear()                                            # frames of one stream share a size: keep one
            cache[key] = Renderer(resolution=key, orig_img=True, wire=bool(getattr(self.options, "wireframe", 0)),
                                  faces=self.smpl_neutral.faces, device=self.device)
        return cache[key]

    def ragged_renderer(self):
        """The renderer behind the ragged launches (every mesh brings its own frame size: its resolution is not used)."""
        r = self.__dict__.get("_ragged_renderer")
        if r is None:
            from .render import Renderer
            r = self._ragged_renderer = Renderer(resolution=(224, 224), orig_img=True, wire=bool(getattr(self.options, "wireframe", 0)),
                                                 faces=self.smpl_neutral.faces, device=self.device)
        return r

    def overlay_sink(self):
        """What the pictures are written through when --overlay_format jpg or --overlay_video 1 ask for the device JPEG encoder
        (jpeg.OverlaySink, made at the first call and kept: this adaptor's own - a replica group writes through its first adaptor's);
        None: PNG files, as ever."""
        if "_overlay_sink" not in self.__dict__:
            from .jpeg import sink_for
            self._overlay_sink = sink_for(self.options, self.device)
        return self._overlay_sink

    def close_overlays(self):
        """End this adaptor's videos (the end of its stream, or an exception on its way out); without a sink nothing happens."""
        close_overlays([self])

    def overlay_videos(self, jobs, name, prefix=None):
        """One entry per job of ``overlay_jobs(...)`` for the same batch: the video a job's picture is appended to with
        --overlay_video 1, ``exppath/video/{prefix}_{sequence name}.avi`` - the name the driver gave this adaptor's sequence
        (``sequence_name``), else the folder of the frame's file, else 'sequence' - and None for a side-view half (it has no picture
        of its own) or without the flag."""
        if not int(getattr(self.options, "overlay_video", 0) or 0):
            return [None] * len(jobs)
        names = [name] if isinstance(name, str) else (list(name) if name is not None else [])
        out, i = [], 0
        for j in jobs:
            if j[3] is None:
                out.append(None)
                continue
            n = names[i] if i < len(names) else None
            i += 1
            seq = getattr(self, "sequence_name", None) or (os.path.basename(os.path.dirname(str(n))) if n else "") or "sequence"
            out.append(os.path.join(self.exppath, "video", f"{prefix}_{seq}.avi"))
        return out

    def result_step(self):
        """The number this frame's result files carry: `global_step`, unless the driver numbers them otherwise (the sharded driver
        with several sequences per GPU: the global frame index - its adaptors share one exppath)."""
        n = getattr(self, "_result_step", None)
        return self.global_step if n is None else n

    def overlay_jobs(self, vts, cam, images, name, bbox, prefix=None):
        """The overlays save_results writes for this batch, not drawn yet: [(frame uint8 (H, W, 3) on the device, vertices
        (6890, 3), camera (4,) = (sx, sy, tx, ty), path)] - over the original frame files when they exist, else over the
        de-normalised crops.  A group collects the jobs of all its sequences and draws them in one ragged launch (draw_overlays).
        --side_view DEG: every overlay job is followed by a second one, (white canvas of the frame's size, vertices, the same camera,
        None, model matrix of the turn by DEG about Y) - the right half of the picture written at the first job's path.
        --save_obj 1: ``exppath/mesh/{prefix}_{n}.obj`` is written here, the mesh turned by Rx as the reference exports it (one file
        per frame beside the picture; the reference's single ``demo.obj`` in the working directory, overwritten by every frame,
        is not reproduced)."""
        jobs = self._overlay_jobs(vts, cam, images, name, bbox, prefix)
        if getattr(self.options, "save_obj", 0):
            from .render import turned_vertices, write_obj
            meshdir = os.path.join(self.exppath, "mesh")
            os.makedirs(meshdir, exist_ok=True)
            for j in jobs:
                stem = os.path.splitext(os.path.basename(j[3]))[0]
                write_obj(os.path.join(meshdir, stem + ".obj"), turned_vertices(j[1]), self.ragged_renderer().faces)
        deg = float(getattr(self.options, "side_view", 0) or 0)
        if not deg:
            return jobs
        from .render import side_view_matrix
        model = side_view_matrix(deg, [0, 1, 0])
        white, both = {}, []
        for frame, v, c, path in jobs:
            key = tuple(frame.shape)
            if key not in white:                                     # frames of one size share one canvas: it is only read
                white[key] = torch.full_like(frame, 255)
            both += [(frame, v, c, path), (white[key], v, c, None, model)]
        return both

    def _overlay_jobs(self, vts, cam, images, name, bbox, prefix):
        from .render import convert_crop_cam_to_orig_img
        vts, cam = vts.detach(), cam.detach().float()
        outdir = os.path.join(self.exppath, "image")
        os.makedirs(outdir, exist_ok=True)
        B = vts.shape[0]
        paths = [os.path.join(outdir, f"{prefix}_{self.result_step() + i}.png") for i in range(B)]
        imgdir = getattr(self, "imgdir", None)
        files = [os.path.join(imgdir, n) for n in name] if (name is not None and bbox is not None and imgdir is not None) else None
        if files is not None and all(os.path.isfile(f) for f in files):
            from .datasets import read_image
            bbox = bbox.detach().to(cam.device).float()
            jobs = []
            for i, f in enumerate(files):
                frame = torch.from_numpy(read_image(f)).to(self.device)
                h, w = int(frame.shape[0]), int(frame.shape[1])
                ocam = convert_crop_cam_to_orig_img(cam[i:i + 1], bbox[i:i + 1], w, h)
                jobs.append((frame, vts[i], ocam[0], paths[i]))
            return jobs
        mean = torch.tensor(constants.IMG_NORM_MEAN, device=images.device).view(1, 3, 1, 1)
        std = torch.tensor(constants.IMG_NORM_STD, device=images.device).view(1, 3, 1, 1)
        crops = ((images.detach() * std + mean) * 255.0).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        ccam = torch.stack([cam[:, 0], cam[:, 0], cam[:, 1], cam[:, 2]], 1)
        return [(crops[i], vts[i], ccam[i], paths[i]) for i in range(B)]

    def save_results(self, vts, cam, images, name, bbox, prefix=None):
        """reference base_adaptor.py:429-443: the predicted mesh drawn over its frame, one PNG per frame of the batch at
        ``exppath/image/{prefix}_{global_step + i}.png``.  vts (B, 6890, 3), cam (B, 3) = (s, tx, ty) of the crop, images the
        normalised (B, 3, 224, 224) crops, name / bbox the batch's ``imgname`` / ``bbox`` (cx, cy, h) - both None for a stream
        without image files (the synthetic bundle): the mesh is then drawn over the de-normalised crop with the crop's own camera
        (s, s, tx, ty).  Vertices, camera and frame stay on the device; only the finished picture comes to the host.
        -> the written paths."""
        # one ragged launch per 64 pictures, whatever their sizes (3DPW mixes 1920x1080 and 1080x1920 frames)
        jobs = self.overlay_jobs(vts, cam, images, name, bbox, prefix)
        return draw_overlays(self.ragged_renderer(), jobs, self.RESULT_COLOR, sink=self.overlay_sink(),
                             videos=self.overlay_videos(jobs, name, prefix))

    def write_summaries(self, losses):
        self.last_summaries = losses


def close_overlays(adaptors):
    """End the videos of these adaptors (a wave of a driver: the group writes through its first adaptor's sink, a lone sequence
    through its own).  An adaptor that never made a sink - PNG runs, or the stand-ins of the host tests - is passed over."""
    for a in adaptors:
        sink = getattr(a, "__dict__", {}).get("_overlay_sink")
        if sink is not None:
            sink.close()


def draw_overlays(renderer, jobs, color, sink=None, videos=None):
    """Draw overlay jobs (BaseAdaptor.overlay_jobs, of one adaptor or of all sequences of a group's step) - one ragged launch per 64
    meshes, each over its own frame at its own size - and write the PNGs.  A job without a path (a side view) is the right half of
    the job before it: the two are drawn by the same launch (a launch then draws at most 32 people: 64 descriptors) and joined on
    the device before the one copy to the host.  sink (jpeg.OverlaySink; None: PNG through PIL): the joined pictures of a launch go
    to it in ONE call - JPEG files and / or the sequences' videos, from one device encode; videos: one entry per job
    (BaseAdaptor.overlay_videos), the video a job's picture is appended to or None.  -> the written paths."""
    from PIL import Image
    paths = []
    lo = 0
    while lo < len(jobs):
        hi = min(lo + 64, len(jobs))
        if hi < len(jobs) and jobs[hi][3] is None:                   # a picture's two halves stay in one launch
            hi -= 1
        part = jobs[lo:hi]
        models = [j[4] if len(j) > 4 else None for j in part]
        pics = renderer.render_many([j[0] for j in part], [j[1] for j in part], torch.stack([j[2] for j in part]), color=color,
                                    models=models if any(m is not None for m in models) else None)
        done, names, into = [], [], []
        for k, j in enumerate(part):
            if j[3] is None:
                continue
            pic = pics[k]
            if k + 1 < len(part) and part[k + 1][3] is None:
                pic = torch.cat([pic, pics[k + 1]], 1)
            if sink is None:
                Image.fromarray(pic.cpu().numpy()).save(j[3])
                paths.append(j[3])
            else:
                done.append(pic)
                names.append(j[3])
                into.append(videos[lo + k] if videos is not None else None)
        if done:
            paths += sink.write(done, names, into)
        lo = hi
    return paths
