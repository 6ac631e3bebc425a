"""Online adaptation on OpenPose BODY_25 detections: one video frame plus one detection in, an adapted mesh out - the live path of the
reference, ``dynaboa_webcam.py::Adaptor.online_adaptation`` (:220-337), without the camera capture and the OpenPose wrapper.

    python -m dynaboa_amd.online --frames DIR --detections FILE --out DIR [--use_boa 1 --dynamic_boa 1 --save_video 1 ...]

is the analogue of the reference's ``--capture_mode video``: frames read with PIL in name order, detections from an ``.npz``
(``imgname``, ``keypoints (N, 25, 3)``) or a directory of OpenPose ``*_keypoints.json`` files (first person), per frame a
``Pred_<n>.npz`` (``verts``, ``cam``, ``rotmat``, ``beta``) and - ``--save_video 1`` - the mesh drawn over the frame as a PNG.

The schedule is the reference's (facts the goldens pin; do not "fix" them):
  * ``save_hist`` stores ``history[global_step]`` and THEN increments ``global_step`` (:102-105): frame n of a stream sees n + 1, the
    motion term is on iff n >= interval and reads frame n + 1 - interval - interval - 1 frames back;
  * the lower level has the frame terms only; the upper level adds the motion term (through the fast weights) and the teacher term;
  * the 2-D keypoint term and the motion term supervise joints [:, :25] of the 49 (keypoint set "op25": csrc/losses.hip), the 25
    detections sitting in slots 0..24 of the [B][49][3] keypoint array;
  * the teacher runs in eval mode; its EMA follows every Adam step (only where there is a teacher - the reference calls it
    unconditionally after the main step and would fail without one);
  * ``use_boa 0``: one loss (frame terms), one Adam step, no teacher update;
  * the dynamic loop's extra steps run on the model itself with the motion and teacher terms, gated on the cosine of feature 12.
With ``use_boa 1`` a frame is ONE call of the native stepper (csrc/adapt_step.hip, the "full" schedule with ``kp_set`` op25,
``metrics`` 0 and no ground-truth pointers) wherever ``native_step.coverage`` allows; ``use_boa 0`` and ``--native_step 0`` run the
autograd composition of the same kernels."""
from __future__ import annotations

import argparse
import glob
import json
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import benchmark as DB
from . import constants as C
from . import datasets as D

parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
# the reference's flag set (dynaboa_webcam.py:339-371) with its defaults
parser.add_argument('--test_basemodel', type=int, default=0, help='also return the un-adapted base model\'s mesh')
parser.add_argument('--save_video', type=int, default=0, help='driver: write the overlay of every frame as a PNG')
parser.add_argument('--res_dir', type=str, default='temp')
parser.add_argument('--seed', type=int, default=22)
parser.add_argument('--model_file', type=str, default='data/basemodel.pt')
parser.add_argument('--lr', type=float, default=3e-6)
parser.add_argument('--beta1', type=float, default=0.5)
parser.add_argument('--beta2', type=float, default=0.9)
parser.add_argument('--use_boa', type=int, default=0)
parser.add_argument('--fastlr', type=float, default=8e-6)
parser.add_argument('--s2dloss_weight', type=float, default=10)
parser.add_argument('--shape_prior_weight', type=float, default=2e-6)
parser.add_argument('--pose_prior_weight', type=float, default=1e-4)
parser.add_argument('--use_meanteacher', type=int, default=1, choices=[0, 1])
parser.add_argument('--alpha', type=float, default=0.1)
parser.add_argument('--teacherloss_weight', type=float, default=0.1)
parser.add_argument('--use_motion', type=int, default=1, choices=[0, 1])
parser.add_argument('--interval', type=int, default=5)
parser.add_argument('--motionloss_weight', type=float, default=0.8)
parser.add_argument('--dynamic_boa', type=int, default=0, choices=[0, 1])
parser.add_argument('--cos_sim_threshold', type=float, default=3.1e-4)
parser.add_argument('--optim_steps', type=int, default=7)
# this build's
parser.add_argument('--native_step', type=int, default=1, choices=[0, 1], help='0: always the autograd composition')
parser.add_argument('--log_frames', type=int, default=256, help='frames of loss / gate log the native stepper keeps (a ring)')
parser.add_argument('--frames', type=str, default=None, help='driver: directory of frames (read in name order)')
parser.add_argument('--detections', type=str, default=None,
                    help='driver: .npz with imgname and keypoints (N, 25, 3), or a directory of OpenPose *_keypoints.json files')
parser.add_argument('--out', type=str, default=None, help='driver: output directory')
parser.add_argument('--one_euro', type=int, default=0, choices=[0, 1],
                    help="1: a causal One-Euro filter (dynaboa_amd.smooth.OneEuro) over the frames' pose, shape and frame camera: results "
                         'gain vts_smooth / rotmat_smooth / shape_smooth (and cam_frame_smooth where box and frame size are known)')
parser.add_argument('--one_euro_min_cutoff', type=float, default=1.0, help='--one_euro 1: cutoff frequency at rest, Hz (lower: smoother)')
parser.add_argument('--one_euro_beta', type=float, default=0.0, help='--one_euro 1: how fast the cutoff grows with speed (higher: less lag)')
parser.add_argument('--fps', type=float, default=30.0, help='--one_euro 1: frame rate of the stream')
parser.add_argument('--track', type=int, default=0, choices=[0, 1],
                    help='driver, with --detections an OpenPose directory: 0: people[0] of every frame; 1: ALL people go through the '
                         'device tracker (dynaboa_amd.track) and every kept track is adapted on its own, from a fresh adaptation '
                         'state, into <out>/track<id>/ (the tracks\' detections: <out>/track<id>.npz, <out>/tracks.json)')
parser.add_argument('--min_track_frames', type=int, default=1, help='--track 1: drop tracks with fewer frames')
from .track import add_rule_arguments as _rule_arguments             # --c_min / --kappa / --s_min / --max_age / --min_common
_rule_arguments(parser)
from .jpeg import add_arguments as _overlay_arguments, sink_for      # --overlay_format / --jpeg_* / --overlay_video / --video_fps
_overlay_arguments(parser)

SCALE_FACTOR = 1.2          # online_adaptation's call of dataprocess (dynaboa_webcam.py:222)
_REFERENCE_FLAGS = ('seed', 'model_file', 'lr', 'beta1', 'beta2', 'use_boa', 'fastlr', 's2dloss_weight', 'shape_prior_weight',
                    'pose_prior_weight', 'use_meanteacher', 'alpha', 'teacherloss_weight', 'use_motion', 'interval', 'motionloss_weight',
                    'dynamic_boa', 'cos_sim_threshold', 'optim_steps', 'native_step')


def online_options(**over):
    """The reference's defaults (``use_boa 0``, ``dynamic_boa 0``, ...) with `over` applied."""
    o = parser.parse_args([])
    for k, v in over.items():
        if not hasattr(o, k):
            raise ValueError(f"unknown option {k}")
        setattr(o, k, v)
    return o


def schedule_options(o):
    """The online flag set as options of the level code (BaseAdaptor._level / the native stepper): one lower level with the frame
    terms, the upper level with motion + teacher, no retrieval, no labelled exemplars, no ground truth, keypoint set op25."""
    s = DB.parser.parse_args([])
    for k in _REFERENCE_FLAGS:
        setattr(s, k, getattr(o, k))
    for k, v in dict(inner_step=1, retrieval=0, lower_level_mixtrain=0, upper_level_mixtrain=0, use_frame_losses_lower=1,
                     use_frame_losses_upper=1, use_temporal_losses_lower=0, use_temporal_losses_upper=1, batch_size=1, sample_num=1,
                     kp_set="op25", metrics=0, eval_lower=0, deferred_metrics=1, overlap_metrics=0, save_res=0, dump_predictions=0,
                     second_order=0).items():
        setattr(s, k, v)
    s.test_basemodel = int(getattr(o, "test_basemodel", 0))
    s.log_frames = int(getattr(o, "log_frames", 256))
    if not s.use_meanteacher and not s.use_motion:
        s.use_temporal_losses_upper = 0
    return s


def bbox_center_scale(kp25, scaleFactor=1.0):
    """dataprocess's box (dynaboa_webcam.py:199-203): over ALL 25 rows - undetected (0, 0, 0) rows included, as the reference does -,
    scale = scaleFactor * max(w, h) / 200.  Evaluated in double.  -> (center [2], scale, bbox (cx, cy, scale * 200))."""
    kp = np.asarray(kp25, dtype=np.float64)
    x0, y0, x1, y1 = kp[:, 0].min(), kp[:, 1].min(), kp[:, 0].max(), kp[:, 1].max()
    center = [(x1 + x0) / 2, (y1 + y0) / 2]
    scale = scaleFactor * max(x1 - x0, y1 - y0) / 200
    return center, scale, np.stack([center[0], center[1], scale * 200])


def process_keypoints(kp25, center, scale):
    """dataprocess's keypoint half (:206-210): confidence > 0.3 -> {0, 1}, positions through the integer-rounding ``transform`` into
    the crop and to [-1, 1].  -> float32 (25, 3)."""
    kp = np.array(kp25, dtype=np.float64)
    kp[:, 2] = kp[:, 2] > 0.3
    return D.j2d_processing(kp, center, scale)


class OnlineAdaptor(DB.Adaptor):
    """``OnlineAdaptor(options)``: options from ``online.parser`` / ``online_options``.  ``assets_bundle``: a synthetic bundle
    (base_adaptor.synthetic_bundle) instead of the checkpoint / SMPL / prior files."""

    def __init__(self, options, assets_bundle=None, device=None):
        self.online_options = options
        super().__init__(schedule_options(options), assets_bundle, device)
        self.model.eval()
        self.basemodel = None
        if self.options.test_basemodel:
            from .hmr import hmr
            self.basemodel = hmr(self._mean_params(), seed=0).to(self.device)
            ck = self._checkpoint()["model"]
            self.basemodel.load_state_dict({k.replace("module.", ""): v for k, v in ck.items()}, strict=True)
            self.basemodel.eval()
        self.reset_records(max(1, self.options.log_frames))
        self.last_extra_steps = 0
        self.one_euro = make_one_euro(options, 1, self.device)    # None without --one_euro 1; reload() leaves it alone (OneEuro.reset)

    def set_dataloader(self):
        self.dataloader = None                    # frames arrive one at a time through online_adaptation()

    # ------------------------------------------------------------------ history: reference dynaboa_webcam.py:98-105
    def save_hist(self, image, s2d):
        self.history[self.global_step] = {"image": image.detach(), "s2d": s2d.detach()}
        self.history.pop(self.global_step - self.options.interval, None)       # (the next frame reads global_step + 1 - interval at the earliest)
        self.global_step += 1

    # ------------------------------------------------------------------ frame + detection -> crop + keypoints
    def dataprocess(self, frame_u8, kp25, scaleFactor=1.0):
        """reference :197-217.  frame_u8: (H, W, 3) uint8 RGB, numpy or tensor (uploaded if it is not on the device yet); kp25: (25, 3)
        OpenPose BODY_25 (x, y, confidence) in frame pixels.  -> (image (1, 3, 224, 224) normalised crop, keypoints (1, 49, 3) with the
        25 detections in slots 0..24, bbox (1, 3) float32 (cx, cy, scale * 200)) - all three on the device."""
        kp25 = np.asarray(kp25.detach().cpu().numpy() if torch.is_tensor(kp25) else kp25)
        if kp25.shape != (25, 3):
            raise ValueError(f"expected one BODY_25 detection (25, 3), got {kp25.shape}")
        center, scale, bbox = bbox_center_scale(kp25, scaleFactor)
        kp = process_keypoints(kp25, center, scale)
        kp49 = torch.zeros(1, C.NUM_OUT_JOINTS, 3)
        kp49[0, :25] = torch.from_numpy(kp)
        frame = frame_u8 if torch.is_tensor(frame_u8) else torch.from_numpy(np.ascontiguousarray(frame_u8))
        image = D.preprocess_frame(frame.to(self.device, non_blocking=True), center, scale)
        bbox = torch.from_numpy(bbox[None, :].astype(np.float32))
        return image.unsqueeze(0), kp49.to(self.device, non_blocking=True), bbox.to(self.device, non_blocking=True)

    # ------------------------------------------------------------------ the frame step
    def inference(self, batch, model, need_feature=False, tag=None, _step=None, _pred=None):
        """The online path has no ground truth: an inference is the forward alone (reference :324-327); the one behind the last
        optimiser step of the frame is what online_adaptation returns."""
        with torch.no_grad():
            out = _pred if (_pred is not None and not need_feature) else model(batch["image"], need_feature)
        if tag is None or tag[0] == "final":
            self._last_pred = (out[0].detach(), out[1].detach(), out[2].detach())
        res = (None, None, None)
        return res + (out[3],) if need_feature else res

    def _native_records(self, slot, nfinal):
        return (None, None, None)                 # metrics = 0: the stepper writes no records

    def _adapt_native(self, batch):
        if self._native is not None:
            self._native.frame %= self._nframes   # the stepper's loss / gate logs are a ring of log_frames frames (views stay valid)
        out = super()._adapt_native(batch)
        ns = self._native
        st = ns.output(1)
        self._last_pred = (ns.output(0).view(1, 24, 3, 3), st[:, 144:154], st[:, 154:157])
        self._last_vts = ns.output(2)
        return out

    def online_adaptation(self, frame_u8, kp25) -> Dict[str, object]:
        """One frame: crop, adapt, infer.  -> {'vts' (1, 6890, 3), 'cam' (1, 3), 'bbox' (1, 3)} - device tensors, valid until the
        next call - plus 'rotmat' / 'shape' of the same inference, and 'vts_base' / 'cam_base' with test_basemodel."""
        image, kp, bbox = self.dataprocess(frame_u8, kp25, scaleFactor=SCALE_FACTOR)
        return self.adapt_processed(image, kp, bbox, frame_size=(int(frame_u8.shape[1]), int(frame_u8.shape[0])))

    def adapt_processed(self, image, kp, bbox=None, frame_size=None) -> Dict[str, object]:
        """online_adaptation behind dataprocess: image (1, 3, 224, 224), kp (1, 49, 3) with the detections in slots 0..24.
        frame_size = (width, height) of the frame the box lies in: with --one_euro 1 it is what the frame camera needs."""
        self.fit_losses = {}
        self.kp2dlosses_lower.clear()
        step = self.global_step
        for d in (self.kp2dlosses_upper, self.feat_sims):            # per-frame logs of a stream without end: keep the newest only
            for k in [k for k in d if k < step]:
                del d[k]
        del self.optim_step_record[:-1]
        self._last_pred = self._last_vts = None
        self.model.eval()
        batch = dict(image=image, smpl_j2d=kp)
        self.adaptation(batch)                    # save_hist, then the native stepper or the autograd composition
        self.last_extra_steps = int(getattr(self, "optimized_step", 0)) if self.options.dynamic_boa and self.options.use_boa else 0
        rot, shape, cam = self._last_pred
        vts = self._last_vts
        if vts is None:
            with torch.no_grad():
                vts = self.decode_smpl_params(rot, shape)["vts"]
        res = dict(vts=vts, cam=cam, bbox=bbox, rotmat=rot, shape=shape)
        if self.basemodel is not None:
            with torch.no_grad():
                b_rot, b_shape, b_cam = self.basemodel(image)
                res.update(vts_base=self.decode_smpl_params(b_rot, b_shape)["vts"], cam_base=b_cam)
        if self.one_euro is not None:
            one_euro_results(self.one_euro, [res], [frame_size], self.decode_smpl_params)
        self.write_summaries(self.fit_losses)
        return res

    def reload(self):
        """reference :184-195: the checkpoint into the model and the teacher, a fresh Adam.  History and the step counter stay.  All in
        place: the native stepper keeps addressing the same weights / moments, and its Adam step count is reset with them."""
        ck = self._checkpoint()["model"]
        plain = {k.replace("module.", ""): v for k, v in ck.items()}
        with torch.no_grad():
            self.model.load_state_dict(ck if self.options.use_boa else plain, strict=True)
            if self.options.use_meanteacher:
                self.teacher.load_state_dict(plain, strict=True)
        for p in self.model.parameters():
            st = self.optimizer.state.get(p)
            if st:
                st["exp_avg"].zero_(); st["exp_avg_sq"].zero_()
                st["step"] = 0
        ns = getattr(self, "_native", None)
        if ns is not None:
            from ._abi import check
            # this sequence's count alone: in an OnlineGroup the stepper is shared, and the other sequences keep theirs
            key = f"adam_step_{getattr(self, '_native_replica', 0)}".encode()
            check(ns.lib.dyb_stepper_set_i(ns.h, key, 0), "set_i " + key.decode())
            ns._sync_adam_steps()

    # ------------------------------------------------------------------ overlay
    def render(self, result, frame_u8, base=False, smooth=False):
        """The mesh of `result` drawn over its frame (render.py; reference utils/webcam_utils.render) -> (H, W, 3) uint8 device tensor.
        smooth=True (--one_euro 1): the filtered mesh, under the filtered frame camera where the result has one."""
        from .render import convert_crop_cam_to_orig_img
        frame = frame_u8 if torch.is_tensor(frame_u8) else torch.from_numpy(np.ascontiguousarray(frame_u8))
        frame = frame.to(self.device)
        h, w = int(frame.shape[0]), int(frame.shape[1])
        if smooth and base:
            raise ValueError("render: the base model's mesh is not filtered - smooth or base, not both")
        if smooth and "vts_smooth" not in result:
            raise ValueError("render(smooth=True) draws the keys that --one_euro 1 adds to a result: this one has none")
        vts, cam = (result["vts_base"], result["cam_base"]) if base else (result["vts_smooth" if smooth else "vts"], result["cam"])
        if smooth and "cam_frame_smooth" in result:
            ocam = result["cam_frame_smooth"].detach().float()
        else:
            ocam = convert_crop_cam_to_orig_img(cam.detach().float(), result["bbox"], w, h)
        color = (100 / 255.0, 100 / 255.0, 200 / 255.0) if base else self.RESULT_COLOR
        return self._renderer(w, h).render(frame, vts.detach()[0], ocam[0], color=color)


def make_one_euro(options, n_seq, device):
    """The filter of --one_euro 1 over `n_seq` sequences (None without the flag): 24 joint rotations, 10 betas and the four
    channels of the frame camera (sx, sy, tx, ty)."""
    if not int(getattr(options, "one_euro", 0)):
        return None
    from .smooth import OneEuro
    return OneEuro(n_seq, fps=float(getattr(options, "fps", 30.0)), min_cutoff=float(getattr(options, "one_euro_min_cutoff", 1.0)),
                   beta=float(getattr(options, "one_euro_beta", 0.0)), J=24, nb=10, nc=4, device=device)


def one_euro_results(filt, results, frame_sizes, decode):
    """One filter step (ONE launch) over the results of all the filter's sequences; every result gains ``rotmat_smooth``,
    ``shape_smooth``, ``vts_smooth`` and - where its box and frame size are known - ``cam_frame_smooth`` (1, 4).  The filter's camera
    channels carry the frame camera (``render.convert_crop_cam_to_orig_img``): the crop camera belongs to the frame's own box, which
    jitters too.  A sequence without box or frame size feeds (s, s, tx, ty) of its crop camera instead and gains no camera key."""
    from .render import convert_crop_cam_to_orig_img
    cams, known = [], []
    for res, size in zip(results, frame_sizes):
        cam = res["cam"].detach().float()
        ok = res.get("bbox") is not None and size is not None
        cams.append(convert_crop_cam_to_orig_img(cam, res["bbox"], size[0], size[1]) if ok else cam[:, [0, 0, 1, 2]])
        known.append(ok)
    rot, shape, camf = filt.step(torch.cat([r["rotmat"].detach().reshape(1, 24, 3, 3) for r in results]),
                                 torch.cat([r["shape"].detach().reshape(1, 10) for r in results]), torch.cat(cams))
    with torch.no_grad():
        vts = decode(rot, shape)["vts"]
    for k, res in enumerate(results):
        res.update(rotmat_smooth=rot[k:k + 1], shape_smooth=shape[k:k + 1], vts_smooth=vts[k:k + 1])
        if known[k]:
            res["cam_frame_smooth"] = camf[k:k + 1]


class OnlineGroup:
    """Several online sequences on ONE GPU in lockstep - several cameras, one frame each per step (native_step.ReplicaGroup: every launch
    of the frame step covers all of them, each with its own weights, Adam state, teacher and history).  The adaptors need ``use_boa 1``
    and identical options, and step together from their first frame on: EVERY sequence brings a frame and a detection to every step
    (one frame counter, one history position and one set of active terms for the whole launch).  A camera without a detected person
    has nothing to adapt on: the caller holds the step back for all of them, or runs that camera as an OnlineAdaptor of its own."""

    def __init__(self, adaptors: Sequence[OnlineAdaptor]):
        from . import native_step as NS
        self.adaptors = list(adaptors)
        self.group = NS.ReplicaGroup(self.adaptors, self.adaptors[0]._nframes)
        # --one_euro 1: ONE filter over all the group's sequences (one launch per step); the adaptors' own filters stay unused
        self.one_euro = make_one_euro(self.adaptors[0].online_options, len(self.adaptors), self.adaptors[0].device)

    def step(self, frames, detections) -> List[Dict[str, object]]:
        """frames[r] / detections[r]: sequence r's frame and BODY_25 detection.  -> one online_adaptation result per sequence."""
        if len(frames) != len(self.adaptors) or len(detections) != len(self.adaptors) or any(
                f is None or d is None for f, d in zip(frames, detections)):
            raise ValueError("every sequence of a group brings a frame and a detection to every step")
        return self.step_processed([a.dataprocess(f, d, scaleFactor=SCALE_FACTOR) + ((int(f.shape[1]), int(f.shape[0])),)
                                    for a, f, d in zip(self.adaptors, frames, detections)])

    def step_processed(self, items) -> List[Dict[str, object]]:
        """items[r] = (image (1, 3, 224, 224), kp (1, 49, 3), bbox (1, 3) or None) of sequence r, optionally followed by the frame's
        (width, height) - what --one_euro 1 needs for the frame camera."""
        ads, ns = self.adaptors, self.group.stepper
        if len(items) != len(ads) or any(it is None for it in items):
            raise ValueError("every sequence of a group brings a frame and a detection to every step")
        active = list(range(len(ads)))
        steps = {a.global_step for a in ads}
        if len(steps) > 1:
            raise ValueError(f"sequences of a group step together: their frame counters differ ({sorted(steps)})")
        ns.frame %= ads[0]._nframes
        for r in active:
            a = ads[r]
            a.kp2dlosses_lower.clear()
            for d in (a.kp2dlosses_upper, a.feat_sims):
                for k in [k for k in d if k < a.global_step]:
                    del d[k]
            del a.optim_step_record[:-1]
            a.model.eval()
        self.group.step([dict(image=it[0], smpl_j2d=it[1]) for it in items], steps.pop())
        out: List[Dict[str, object]] = [{}] * len(items)
        for r in active:
            a, st = ads[r], ns.output(1, r)
            a.last_extra_steps = int(getattr(a, "optimized_step", 0)) if a.options.dynamic_boa else 0
            if a.options.dynamic_boa:
                # sequences leave the dynamic loop after different numbers of steps, and the stepper's two activation arenas swap roles
                # every step: which one holds THIS sequence's last inference is not exposed - one forward at its adapted weights
                with torch.no_grad():
                    rot, shape, cam = a.model(items[r][0])
                    res = dict(vts=a.decode_smpl_params(rot, shape)["vts"], cam=cam, bbox=items[r][2], rotmat=rot, shape=shape)
            else:
                res = dict(vts=ns.output(2, r), cam=st[:, 154:157], bbox=items[r][2], rotmat=ns.output(0, r).view(1, 24, 3, 3),
                           shape=st[:, 144:154])
            if a.basemodel is not None:
                with torch.no_grad():
                    b_rot, b_shape, b_cam = a.basemodel(items[r][0])
                    res.update(vts_base=a.decode_smpl_params(b_rot, b_shape)["vts"], cam_base=b_cam)
            a.write_summaries(a.fit_losses)
            out[r] = res
        if self.one_euro is not None:
            one_euro_results(self.one_euro, out, [it[3] if len(it) > 3 else None for it in items], ads[0].decode_smpl_params)
        return out


# ---------------------------------------------------------------------------------------- the driver
def load_detections(path: str, frame_names: Optional[Sequence[str]] = None) -> Dict[str, np.ndarray]:
    """-> {frame file name: (25, 3) float array}.  `path`: an .npz with ``imgname`` and ``keypoints (N, 25, 3)``, or a directory of
    OpenPose per-frame ``<frame stem>_keypoints.json`` files (``people[0].pose_keypoints_2d``; a frame without a person is left out)."""
    if os.path.isdir(path):
        out = {}
        stems = {os.path.splitext(n)[0]: n for n in (frame_names or [])}
        for f in sorted(glob.glob(os.path.join(path, "*_keypoints.json"))):
            stem = os.path.basename(f)[:-len("_keypoints.json")]
            with open(f) as fh:
                people = json.load(fh).get("people", [])
            if people:
                out[stems.get(stem, stem)] = np.asarray(people[0]["pose_keypoints_2d"], dtype=np.float32).reshape(25, 3)
        return out
    z = np.load(path, allow_pickle=False)
    kps = np.asarray(z["keypoints"], dtype=np.float32)
    if kps.ndim != 3 or kps.shape[1:] != (25, 3):
        raise ValueError(f"{path}: keypoints must be (N, 25, 3), got {kps.shape}")
    return {os.path.basename(str(n)): kps[i] for i, n in enumerate(z["imgname"])}


def run_driver(options, adaptor: Optional[OnlineAdaptor] = None, assets_bundle=None, device=None) -> List[str]:
    """Frames of ``--frames`` in name order through online_adaptation; a frame without a detection is skipped, as the reference's loop
    does on its TypeError (:420).  <n> of Pred_<n> is the frame's position in the name-ordered listing, skipped frames counted (the
    reference numbers its outputs by a counter of the frames it read, likewise) - a skipped frame leaves a gap.  -> the Pred_<n>.npz
    paths written."""
    from PIL import Image
    if not (options.frames and options.detections and options.out):
        raise SystemExit("--frames, --detections and --out are required")
    names = sorted(n for n in os.listdir(options.frames) if n.lower().endswith((".png", ".jpg", ".jpeg", ".bmp")))
    if int(getattr(options, "track", 0)):
        return run_tracked(options, names, adaptor, assets_bundle, device)
    dets = load_detections(options.detections, names)
    ad = adaptor if adaptor is not None else OnlineAdaptor(options, assets_bundle, device)
    return drive_frames(options, names, dets, ad, options.out)


def run_tracked(options, names: Sequence[str], adaptor=None, assets_bundle=None, device=None) -> List[str]:
    """--track 1: the people of an OpenPose directory through ``track.track_openpose`` (-> ``<out>/track<id>.npz``,
    ``<out>/tracks.json``), then every kept track through ``drive_frames`` with an adaptor of its own - what the driver does on that
    track's file alone - into ``<out>/track<id>/``, one track after the other.  (Stepping the people of one camera as an
    ``OnlineGroup`` is not done here: a group's sequences must all start at frame 0 and bring a detection to every step.)"""
    from . import track as T
    if not os.path.isdir(options.detections):
        raise ValueError("--track 1 reads a directory of OpenPose *_keypoints.json files (--detections DIR): an .npz holds one person "
                         "per frame already")
    if adaptor is not None:
        raise ValueError("--track 1 adapts every track from a fresh adaptation state: it builds its adaptors itself")
    paths = T.track_openpose(options.detections, options.out, names, int(getattr(options, "min_track_frames", 1)),
                             device="cuda" if device is None else device, **T.rule_of(options))
    written = []
    for t, path in paths.items():
        ad = OnlineAdaptor(options, assets_bundle, device)
        written += drive_frames(options, names, load_detections(path, names), ad, os.path.join(options.out, f"track{t}"))
    return written


def drive_frames(options, names: Sequence[str], dets: Dict[str, np.ndarray], ad: OnlineAdaptor, out: str) -> List[str]:
    """The driver's loop: the frames `names` of ``--frames`` that have a detection through `ad` -> ``<out>/Pred_<n>...``."""
    from PIL import Image
    os.makedirs(out, exist_ok=True)
    # --overlay_format jpg: Pred_{n}.jpg from the device encoder; --overlay_video 1: Pred.avi beside the pictures (and, with
    # --one_euro 1, Pred_smooth.avi of the filtered mesh) - either makes the driver draw, as --save_video 1 does
    sink = sink_for(options, ad.device)
    video = sink is not None and sink.video
    written = []
    try:
        for n, name in enumerate(names):
            if name not in dets:
                continue
            frame = D.read_image(os.path.join(options.frames, name))
            res = ad.online_adaptation(frame, dets[name])
            cam = res["cam"].detach()
            cam_t = torch.stack([cam[:, 1], cam[:, 2], 2 * C.FOCAL_LENGTH / (C.IMG_RES * cam[:, 0] + 1e-9)], dim=-1)
            path = os.path.join(out, f"Pred_{n}.npz")
            np.savez(path, verts=res["vts"].detach().cpu().numpy(), cam=cam_t.cpu().numpy(), rotmat=res["rotmat"].cpu().numpy(),
                     beta=res["shape"].cpu().numpy())
            written.append(path)
            if sink is None:
                if options.save_video:
                    Image.fromarray(ad.render(res, frame).cpu().numpy()).save(os.path.join(out, f"Pred_{n}.png"))
                continue
            pics, paths, videos = [], [], []
            if options.save_video or video:
                pics.append(ad.render(res, frame))
                paths.append(os.path.join(out, f"Pred_{n}.png") if options.save_video else None)
                videos.append(os.path.join(out, "Pred.avi"))
            if video and "vts_smooth" in res:
                pics.append(ad.render(res, frame, smooth=True))
                paths.append(None)
                videos.append(os.path.join(out, "Pred_smooth.avi"))
            if pics:
                sink.write(pics, paths, videos)
    finally:
        if sink is not None:
            sink.close()
    return written


if __name__ == '__main__':
    run_driver(parser.parse_args())
