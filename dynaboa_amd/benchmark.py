"""Drop-in for reference ``dynaboa_benchmark.py``: the same argparse flags (:16-65) and an
``Adaptor`` with ``excute() / adaptation(batch) / inference(batch, model)`` running the same
per-frame bilevel schedule (:126-193) and metric path (:204-262) on the HIP kernels.

Differences that do not change results:
  * per-inference ``joblib.dump`` of 6890x3 vertices (:250-254) is off unless --dump_predictions 1;
  * with --deferred_metrics 1 the 14-joint sets are kept on the device and the Procrustes kernel runs once over
    the whole stream instead of forcing a host sync four times per frame;
  * forwards the schedule repeats with identical weights and input are evaluated once (--share_forwards), and each
    level's model -> SMPL -> loss head is one autograd node (--fused_level).
"""
from __future__ import annotations

import argparse
import os
import queue
import re
import threading
from typing import Dict, Iterable, Optional

import numpy as np
import torch

from . import _lib
from . import pose_utils as PU
from ._abi import check
from .base_adaptor import BaseAdaptor
from .hmr import stream_of
from .pose_utils import compute_similarity_transform_batch, pa_mpjpe_device  # noqa: F401  (the NumPy form stays importable from here, as in the reference)

parser = argparse.ArgumentParser()
parser.add_argument('--expdir', type=str, default='exps')
parser.add_argument('--expname', type=str, default='3dpw')
parser.add_argument('--dataset', type=str, default='3dpw', choices=['3dpw', 'internet'])
parser.add_argument('--seed', type=int, default=22)
parser.add_argument('--seq_seed', type=int, default=22)
parser.add_argument('--model_file', type=str, default='data/basemodel.pt')
parser.add_argument('--batch_size', type=int, default=1)
parser.add_argument('--save_res', type=int, default=0, choices=[0, 1])
parser.add_argument('--side_view', type=float, default=0.0,
                    help='with --save_res 1: DEG != 0 makes every picture a panel of twice the width - the overlay on the left, the mesh '
                         'turned by DEG degrees about Y over a white canvas on the right, under the same camera (270 is the usual choice)')
parser.add_argument('--wireframe', type=int, default=0, choices=[0, 1],
                    help='with --save_res 1: draw the overlay (and the side view) as a wireframe')
parser.add_argument('--save_obj', type=int, default=0, choices=[0, 1],
                    help='with --save_res 1: also write mesh/{prefix}_{n}.obj per frame, the mesh turned by 180 degrees about X')
from .jpeg import add_arguments as _overlay_arguments       # --overlay_format / --jpeg_* / --overlay_video / --video_fps
_overlay_arguments(parser)
parser.add_argument('--lr', type=float, default=3e-6)
parser.add_argument('--beta1', type=float, default=0.5)
parser.add_argument('--beta2', type=float, default=0.9)
parser.add_argument('--use_boa', type=int, default=1, choices=[0, 1])
parser.add_argument('--fastlr', type=float, default=8e-6)
parser.add_argument('--inner_step', type=int, default=1)
parser.add_argument('--record_lowerlevel', type=int, default=1)
parser.add_argument('--s2dloss_weight', type=float, default=10)
parser.add_argument('--shape_prior_weight', type=float, default=2e-6)
parser.add_argument('--pose_prior_weight', type=float, default=1e-4)
parser.add_argument('--use_frame_losses_lower', type=int, default=1, choices=[0, 1])
parser.add_argument('--use_frame_losses_upper', type=int, default=1, choices=[0, 1])
parser.add_argument('--use_temporal_losses_lower', type=int, default=0, choices=[0, 1])
parser.add_argument('--use_temporal_losses_upper', type=int, default=1, choices=[0, 1])
parser.add_argument('--sample_num', type=int, default=1)
parser.add_argument('--retrieval', type=int, default=1, choices=[0, 1])
parser.add_argument('--dynamic_boa', type=int, default=1, choices=[0, 1])
parser.add_argument('--cos_sim_threshold', type=float, default=3.1e-4)
parser.add_argument('--optim_steps', type=int, default=7)
parser.add_argument('--lower_level_mixtrain', type=int, default=1, choices=[0, 1])
parser.add_argument('--upper_level_mixtrain', type=int, default=1, choices=[0, 1])
parser.add_argument('--mixtrain', type=int)
parser.add_argument('--labelloss_weight', type=float, default=0.1)
parser.add_argument('--use_meanteacher', type=int, default=1, choices=[0, 1])
parser.add_argument('--alpha', type=float, default=0.1)
parser.add_argument('--teacherloss_weight', type=float, default=0.1)
parser.add_argument('--use_motion', type=int, default=1, choices=[0, 1])
parser.add_argument('--interval', type=int, default=5)
parser.add_argument('--motionloss_weight', type=float, default=0.8)
# additions (not in the reference)
parser.add_argument('--dump_predictions', type=int, default=0, choices=[0, 1])
parser.add_argument('--hvp', type=str, default=os.environ.get("DYB_HVP", "exact"), choices=["fd", "exact"],
                    help='second order only: Hessian-vector products forward-over-reverse through the tangent kernels - exact through '
                         'the backbone and regressor; the 157-input loss head (rot6d -> SMPL -> projection / priors) is differentiated '
                         'along the state tangent by a central difference of its analytic gradient (exact: levels made of the frame '
                         'losses; other levels fall back) - or as a central difference of first-order gradients of the whole level (fd)')
parser.add_argument('--hvp_head', type=str, default=os.environ.get("DYB_HVP_HEAD", "fd"), choices=["fd", "closed"],
                    help='--second_order 1 --hvp exact only: the second derivative of the 157-input loss head as a central difference of '
                         'its analytic gradient (fd, the default) or in closed form (closed: one dyb_head_hvp call runs every head kernel '
                         'on (value, tangent) pairs - with it the whole product H v is exact, no step size anywhere).  Closed covers levels '
                         'made of the frame losses; a level with teacher / motion / labelled terms keeps fd for its whole head (logged '
                         'once per run)')
parser.add_argument('--hvp_terms', type=str, default="all", choices=["all", "frame"],
                    help='--hvp exact for every level through the multi-pass form (all, the default: on MI355X the 4-frame second-order '
                         'stream on the default term set matches the reference\'s first_order=False run element-wise) or only for levels '
                         'made of the frame losses (frame: levels with teacher / motion / labelled terms take the difference quotient)')
parser.add_argument('--fused_so_adam', type=int, default=1, choices=[0, 1],
                    help='second order: fold the last accumulation of the outer gradient (v - lr*Hv) into the Adam launch')
parser.add_argument('--second_order', type=int, default=0, choices=[0, 1],
                    help='1: second-order MAML (learn2learn first_order=False); the reference hard-codes first order '
                         '(base_adaptor.py:119).  See dynaboa_amd/maml.py for how the Hessian-vector products are formed')
parser.add_argument('--share_forwards', type=int, default=1, choices=[0, 1],
                    help='1: forwards the reference schedule repeats with identical weights and input (the un-adapted '
                         'feature forward, the inference() after each inner step) reuse the level forward of the same '
                         'weights - identical results, 5 instead of 9 HMR forwards per frame at inner_step 3')
parser.add_argument('--fused_level', type=int, default=1, choices=[0, 1],
                    help='1: model -> SMPL -> frame-loss head of each adaptation level as one autograd node (same results); '
                         '0: the three-module composition')
parser.add_argument('--term_kernels', type=int, default=1, choices=[0, 1],
                    help='autograd path: 1 = the mean-teacher / motion / labelled-exemplar terms as one value+gradient launch each '
                         '(dyb_aux_loss_terms, what the native stepper issues); 0 = composed from torch ops as the reference writes them')
parser.add_argument('--deferred_metrics', type=int, default=0, choices=[0, 1])
parser.add_argument('--overlap_metrics', type=int, default=0, choices=[0, 1, 2],
                    help='with --deferred_metrics 1: run the no-grad metric / feature forwards on a side HIP stream, '
                         'concurrently with the next adaptation step (same arithmetic, same results); 2 = also issue '
                         'them from a second host thread')
parser.add_argument('--bf16_mfma', type=int, default=0, choices=[0, 1],
                    help='1: the backbone convolutions run on the bf16 matrix cores (fp32 master weights, fp32 activations, '
                         'GroupNorm statistics and accumulators; operand tiles rounded to bf16 as they are staged) - the '
                         'fp32-vs-bf16 arm of BASELINE configs[4]; 0 (default): exact fp32, the parity mode')
parser.add_argument('--teacher_dropout', type=int, default=0, choices=[0, 1],
                    help='1: leave the mean teacher in train() mode like the reference does (base_adaptor.py:151-158 never calls '
                         'teacher.eval()): live Dropout(0.5) after fc1 / fc2 in the teacher forward; 0: deterministic teacher')
parser.add_argument('--native_step', type=int, default=1, choices=[0, 1],
                    help='1: configurations the native frame stepper covers (first order, frame-loss set; csrc/adapt_step.hip) '
                         'run as ONE C call per frame - same kernels, same order, identical weights; 0: always the '
                         'torch.autograd composition')
parser.add_argument('--num_shards', type=int, default=1,
                    help="split the stream by sequence over this many processes (1 = the reference's single stream; dynaboa_amd/sharded.py)")
parser.add_argument('--shard_rank', type=int, default=0, help="this process's shard (torchrun's RANK overrides it)")
parser.add_argument('--seqs_per_gpu', type=int, default=1,
                    help="sequences of this shard adapted at once, in lockstep launches (own weights / Adam state / records each)")
parser.add_argument('--replica_policy', choices=['throughput', 'bitexact'], default='throughput',
                    help="--seqs_per_gpu > 1: 'throughput' = split depth chosen for the replica-multiplied grid and, from 5 sequences per "
                         "launch, the throughput schedule (results equal to a sequence adapted alone to fp32 rounding); 'bitexact' = the "
                         "single-sequence policy (bit-identical to sequences adapted alone, about half the frame rate at 32 sequences)")
parser.add_argument('--native_results', type=int, default=0, choices=[0, 1],
                    help='1: --save_res / --dump_predictions stay on the native frame stepper (and work with --seqs_per_gpu > 1): the '
                         'stepper keeps each frame\'s last final inference in a result ring on the device, the overlay of a step\'s frames '
                         'is drawn from there by one ragged launch and the dump is written from there; 0 (default): both take the run '
                         'to the torch.autograd composition')
parser.add_argument('--exemplar_bank', type=int, default=0, choices=[0, 1],
                    help='1 (with a real data tree): the retrieval set is preprocessed once and kept resident on the device (602 KB per '
                         'exemplar); the nearest cluster and the member are picked by HIP kernels from a counter-based generator seeded '
                         'with --seed (same distribution as the reference\'s random.sample, not the same samples) and the native stepper '
                         'retrieves inside the level - no host callback, parallel passes stay on; 0 (default): the reference\'s host retrieval')
parser.add_argument('--eval_lower', type=int, default=1, choices=[0, 1],
                    help='run inference() after every inner step like the reference (:142)')
parser.add_argument('--seq_metrics', type=int, default=0, choices=[0, 1],
                    help='1: besides MPJPE / PA-MPJPE / PVE report the acceleration error, PCK@150mm and AUC of every frame and the means '
                         'of every sequence (reference utils/pose_utils.py: compute_error_accel, reconstruction_error(needpck, needauc)) - '
                         'computed at the metric flush by one dyb_seq_metrics call over all frames; forces --deferred_metrics 1 and writes '
                         '<exppath>/metrics.json and <exppath>/metrics_per_sequence.csv')


def frame_only_options(**over):
    """The 'frame losses only' configuration of SURVEY 8d config 2."""
    o = parser.parse_args([])
    for k, v in dict(retrieval=0, lower_level_mixtrain=0, upper_level_mixtrain=0, use_meanteacher=0, use_motion=0,
                     dynamic_boa=0, use_temporal_losses_upper=0).items():
        setattr(o, k, v)
    for k, v in over.items():
        setattr(o, k, v)
    return o


class _SideWorker(threading.Thread):
    """Issues work for the side HIP stream from its own host thread, so that the ~0.5 ms of launch
    issue per no-grad forward does not serialise with the main thread's (ctypes and torch release the
    GIL while launching).  Tasks run strictly in submission order under the side stream."""

    def __init__(self, device, stream):
        super().__init__(daemon=True)
        self.device, self.stream = device, stream
        self.q: "queue.Queue" = queue.Queue()
        self.error = None
        self.start()

    def run(self):
        torch.cuda.set_device(self.device)
        while True:
            item = self.q.get()
            if item is None:
                return
            fn, fut = item
            try:
                with torch.cuda.stream(self.stream):
                    fut["out"] = fn()
                    ev = torch.cuda.Event()
                    ev.record(self.stream)
                    fut["event"] = ev
            except BaseException as e:      # noqa: BLE001  (re-raised on the main thread at the next join)
                self.error = e
            finally:
                fut["done"].set()

    def submit(self, fn):
        fut = dict(done=threading.Event(), out=None, event=None)
        self.q.put((fn, fut))
        return fut


class Adaptor(BaseAdaptor):
    def reset_records(self, nframes: int):
        if getattr(self.options, "seq_metrics", 0):
            self.options.deferred_metrics = 1         # the joint sets must stay on the device until the flush
        self._frame_names = []                         # --seq_metrics 1: the imgname of every frame, for the frame ids
        self.sims, self.feat_sims, self.optim_step_record = [], {}, []
        self.mpjpe_statistics, self.pampjpe_statistics = [[] for _ in range(nframes)], [[] for _ in range(nframes)]
        self.mpjpe_all_lower = [[] for _ in range(self.options.inner_step)]
        self.pampjpe_all_lower = [[] for _ in range(self.options.inner_step)]
        self.history, self.kp2dlosses_lower, self.kp2dlosses_upper = {}, [], {}
        self._pending = []            # deferred metric records
        self._native, self._native_why, self._nframes = None, None, nframes
        self._side, self._side_done, self._worker, self._last_fut = None, None, None, None
        if getattr(self.options, "overlap_metrics", 0) and self.options.deferred_metrics and self.device.type == "cuda":
            self._side = torch.cuda.Stream(device=self.device)
            if getattr(self.options, "overlap_metrics", 0) >= 2 and not self._native_ok():
                self._worker = _SideWorker(self.device, self._side)

    # ------------------------------------------------------------------ side-stream plumbing
    def _on_side(self, fn, *reads):
        """Run fn() on the side stream after everything issued so far on the current stream.
        `reads`: tensors produced on the main stream that fn reads (kept alive for the side stream).
        With a worker thread the call returns a future-like dict ({'done','out','event'})."""
        if self._side is None:
            return fn()
        ev = torch.cuda.Event()
        ev.record()
        for t in reads:
            if torch.is_tensor(t) and t.is_cuda:
                t.record_stream(self._side)
        if self._worker is not None:
            side = self._side

            def task():
                side.wait_event(ev)
                return fn()
            self._last_fut = self._worker.submit(task)
            return self._last_fut
        self._side.wait_event(ev)
        with torch.cuda.stream(self._side):
            out = fn()
            self._side_done = torch.cuda.Event()
            self._side_done.record(self._side)
        return out

    def _join_side(self):
        """Main stream waits for the side stream (before theta / teacher are modified in place, or
        before side results are consumed on the main stream)."""
        if self._side is None:
            return
        if self._worker is not None:
            if self._last_fut is not None:
                self._last_fut["done"].wait()           # host: the worker has issued everything submitted so far
                if self._worker.error is not None:
                    err, self._worker.error = self._worker.error, None
                    raise err
                self._side_done = self._last_fut["event"]
        if self._side_done is not None:
            torch.cuda.current_stream(self.device).wait_event(self._side_done)

    @staticmethod
    def _resolve(x):
        """Value of something returned by _on_side (after _join_side)."""
        if isinstance(x, dict) and "done" in x and "event" in x:
            x["done"].wait()
            return x["out"]
        return x

    @staticmethod
    def _theta_of(model):
        t = getattr(model, "_theta", None)
        if t is None:
            m = getattr(model, "module", model)
            t = getattr(m, "theta", None)
        return t

    def excute(self, frames: Optional[Iterable[Dict[str, torch.Tensor]]] = None, nframes: Optional[int] = None, seq_lengths=None):
        """`seq_lengths` (--seq_metrics 1): the frame counts of the stream's sequences; None = the loader's dataset's `sequences`
        where the stream is that whole dataset (the single-stream parity mode reports per sequence too), else one sequence."""
        frames = self.dataloader if frames is None else frames
        nframes = len(frames) if nframes is None else nframes
        self.reset_records(nframes)
        seq = bool(getattr(self.options, "seq_metrics", 0))
        if seq:
            self._seq_names = getattr(self, "seq_names", None)          # (a caller that knows its sequences' names sets seq_names)
            ds = getattr(frames, "ds", None)
            if seq_lengths is None and getattr(ds, "sequences", None) and list(getattr(frames, "indices", ())) == list(range(len(ds))):
                seq_lengths = [s["frames"] for s in ds.sequences]
                self._seq_names = [os.path.basename(str(s["file"])) for s in ds.sequences]
            self._seq_lengths = None if seq_lengths is None else [int(v) for v in seq_lengths]
        mpjpe_all, pampjpe_all, pve_all = [], [], []
        try:
            for step, batch in enumerate(frames):
                self.global_step = step
                self.fit_losses = {}
                batch = {k: v.to(self.device) if isinstance(v, torch.Tensor) else v for k, v in batch.items()}
                if seq:
                    self.note_frame_names(batch)
                self.model.eval()
                mpjpe, pampjpe, pve = self.adaptation(batch)
                self.write_summaries(self.fit_losses)
                mpjpe_all.append(mpjpe); pampjpe_all.append(pampjpe); pve_all.append(pve)
        finally:
            self.close_overlays()                              # the stream's videos end with it, also on an exception
        if self.options.deferred_metrics:
            final = self.flush_metrics()
            self.metric_records = final["records"]          # every inference() of the run, incl. the per-inner-step ones
            mpjpe_all, pampjpe_all, pve_all = final["mpjpe"], final["pampjpe"], final["pve"]
        self.results = dict(mpjpe=mpjpe_all, pampjpe=pampjpe_all, pve=pve_all)
        if seq:
            self.results.update({k: final[k] for k in SEQ_KEYS})
            if getattr(self, "_seq_report", True):
                write_sequence_report(self.exppath, self.options, self.results)
        return self.results

    def note_frame_names(self, batch):
        """--seq_metrics 1: remember the frames' imgname (one per sample); the flush reads the frame ids from them."""
        names = batch.get("imgname")
        B = int(batch["image"].shape[0])
        names = [names] if isinstance(names, str) else list(names) if names is not None else []
        self._frame_names.extend(names if len(names) == B else [None] * B)

    # ------------------------------------------------------------------ native frame stepper (csrc/adapt_step.hip)
    def _native_ok(self):
        """Whether frames of this run go through the native stepper (decided once per reset_records)."""
        if self._native_why is None:
            from . import native_step as NS
            if getattr(self.options, "native_step", 1):
                why = NS.coverage(self.options, self.bundle is not None)[1]
            else:
                why = "native_step=0"
            self._native_why = why or ""
        return self._native_why == ""

    def _adapt_native(self, batch):
        from . import native_step as NS
        if self._native is None:
            self._native, self._native_replica = NS.NativeStepper(self, self._nframes), 0
        if self._native.full:
            return self._adapt_native_full(batch)
        f, slot = self._native.adapt_frame(batch, side_stream=self._side)
        out = self._native_bookkeeping(f, slot)
        self._native_write_results(f, batch)
        return out

    def _native_write_results(self, f, batch):
        """--native_results 1: what the autograd path's inference() leaves behind for the frame - result/Pred_{n}.pt and
        image/Pred_{n}.png of its LAST final inference - from the stepper's result ring."""
        ns = self._native
        if ns.results is None:
            return
        ns.join()                                            # a side-stream tail owes this frame's final inference
        res = ns.result(f, getattr(self, "_native_replica", 0))
        if self.options.dump_predictions:
            self.dump_prediction(res["vts"], res["cam"], res["rotmat"], res["shape"])
        if getattr(self.options, "save_res", 0):
            self.save_results(res["vts"], res["cam"], batch["image"], batch.get("imgname"), batch.get("bbox"), prefix="Pred")

    def dump_prediction(self, vts, cam, rotmat, shape):
        """result/Pred_{n}.pt (reference dynaboa_benchmark.py:250-254), n = result_step(): what inference() and the native path write."""
        import joblib
        os.makedirs(os.path.join(self.exppath, 'result'), exist_ok=True)
        cam_t = torch.stack([cam[:, 1], cam[:, 2], 2 * 5000. / (224 * cam[:, 0] + 1e-9)], dim=-1)
        joblib.dump({'verts': vts.cpu().numpy(), 'cam': cam_t.cpu().numpy(), 'rotmat': rotmat.cpu().numpy(), 'beta': shape.cpu().numpy()},
                    os.path.join(self.exppath, 'result', f'Pred_{self.result_step()}.pt'))

    def _native_full_inputs(self, batch):
        """-> (hist, exemplars) of this frame for the native full-term stepper: the history pair of the motion term (None while
        there is no frame `interval` steps back) and the labelled exemplars when they do not depend on the level's feature (the
        synthetic bundle; None = the stepper's retrieval callback asks self.retrieval per level)."""
        o = self.options
        hist = None
        if self.motion_on() and (o.use_temporal_losses_upper or o.use_temporal_losses_lower):
            hist = self.get_hist()
        ex = None
        if (o.lower_level_mixtrain or o.upper_level_mixtrain) and self.bundle is not None:
            ex = self._last_h36m = self.retrieval(None)          # the synthetic bundle's exemplars depend on the step only
        return hist, ex

    def _adapt_native_full(self, batch):
        """The reference's full term set through the native stepper: one C call for the whole frame incl. the dynamic loop."""
        hist, ex = self._native_full_inputs(batch)
        f, slot, extra = self._native.adapt_frame_full(batch, hist, ex)
        out = self._native_full_bookkeeping(f, slot, extra, hist)
        self._native_write_results(f, batch)
        return out

    def _native_full_bookkeeping(self, f, slot, extra, hist):
        """What adaptation() leaves behind after a full-term frame (replica `_native_replica` of the stepper)."""
        o, ns, rr = self.options, self._native, getattr(self, "_native_replica", 0)
        K = o.inner_step
        log = self.fit_losses
        cut = {}                                                 # one slice + one unbind per log row (16 views), not one index op per value

        def lrow(row):
            if row not in cut:
                cut[row] = ns.level_row(f, row, rr).unbind(0)
            return cut[row]
        for i in range(K):
            self.kp2dlosses_lower.append(lrow(i)[0])
        rows = ((("ll", K - 1, bool(o.use_temporal_losses_lower), bool(o.lower_level_mixtrain)),) if K > 0 else ()) + \
               (("ul", K + min(extra, o.optim_steps if o.dynamic_boa else 0), bool(o.use_temporal_losses_upper), bool(o.upper_level_mixtrain)),)
        for tag, row, temporal, mix in rows:
            r = lrow(row)
            log[f"{tag}/s2dloss"], log[f"{tag}/shape_prior"], log[f"{tag}/pose_prior"], log[f"{tag}/unlabelloss"] = r[0], r[1], r[2], r[3]
            if temporal and o.use_meanteacher:
                for j, k in enumerate(("s2dloss", "s3dloss", "shape_loss", "pose_loss", "loss")):
                    log[f"teacher/{k}"] = r[4 + j]
            if temporal and o.use_motion and hist is not None:
                log["ul/motion_loss"] = r[9]
            if mix:
                for j, k in enumerate(("labled_s2dloss", "labled_s3dloss", "labled_shape_loss", "labled_pose_loss", "labled_loss")):
                    log[f"{tag}/{k}"] = r[10 + j]
            log[f"{tag}/total"] = r[15]
        self.kp2dlosses_upper[self.global_step] = lrow(K)[0]
        nfinal = 1 + (min(extra, o.optim_steps) if o.dynamic_boa else 0)
        out = self._native_records(slot, nfinal)
        if o.dynamic_boa:
            cos, means = ns.gate_views(f, rr)                                 # views cut once per frame for all sequences (native_step.py)
            self.feat_sims[self.global_step] = [{i: {"cos": c} for i, c in enumerate(cos[k])} for k in range(nfinal)]
            log["feat_sim/cos_sim"] = means[nfinal - 1]                         # the reference divides by the last index (base_adaptor.py:218)
            self.optimized_step = extra
            self.optim_step_record.append(extra)
        return out

    def _native_bookkeeping(self, f, slot):
        """What adaptation() leaves behind besides the weights: logged losses, metric records, per-step statistics - read
        from the stepper's device buffers (views; nothing synchronises unless deferred_metrics = 0)."""
        o, ns, r = self.options, self._native, getattr(self, "_native_replica", 0)
        K = o.inner_step
        for i in range(K):
            self.kp2dlosses_lower.append(ns.losses(f, i, r)[0])
        log = self.fit_losses
        for tag, lv in ((("ll", K - 1),) if K > 0 else ()) + (("ul", K),):
            l4 = ns.losses(f, lv, r).unbind(0)
            log[f"{tag}/s2dloss"], log[f"{tag}/shape_prior"], log[f"{tag}/pose_prior"] = l4[0], l4[1], l4[2]
            log[f"{tag}/unlabelloss"] = log[f"{tag}/total"] = l4[3]
        self.kp2dlosses_upper[self.global_step] = log["ul/s2dloss"]
        if not o.deferred_metrics:
            ns.join()
        return self._native_records(slot, 1)

    def _native_records(self, slot, nfinal):
        """The frame's metric records from the stepper's device buffers, in schedule order from `slot`: one per inner step (eval_lower),
        then `nfinal` final inferences (> 1: the dynamic loop's) -> the last final one's (mpjpe, pampjpe, pve)."""
        o, ns, r = self.options, self._native, getattr(self, "_native_replica", 0)
        out = (None, None, None)
        tags = ([('lower', i) for i in range(o.inner_step)] if getattr(o, "eval_lower", 1) else []) + [('final', k) for k in range(nfinal)]
        stats_m, stats_p = [], []
        for tag in tags:
            v = ns.record_views(slot, r)
            slot += 1
            if o.deferred_metrics:
                self._pending.append(dict(step=self.global_step, tag=tag, **v))
                res = (v["mpjpe"], None, v["pve"])
            else:
                pa = pa_mpjpe_device(v["pred"], v["gt"]).cpu().numpy()
                res = (v["mpjpe"].cpu().numpy() * 1000, pa * 1000, float(v["pve"]) * 1000)
            if tag[0] == 'lower':
                self.mpjpe_all_lower[tag[1]].append(res[0]); self.pampjpe_all_lower[tag[1]].append(res[1])
            else:
                out = res
                stats_m.append(res[0]); stats_p.append(res[1])
        if self.global_step < len(self.mpjpe_statistics):
            self.mpjpe_statistics[self.global_step], self.pampjpe_statistics[self.global_step] = stats_m, stats_p
        return out

    # ------------------------------------------------------------------ the per-frame bilevel step
    def adaptation(self, batch):
        o = self.options
        image, gt_keypoints_2d = batch['image'], batch['smpl_j2d']
        self.save_hist(image, gt_keypoints_2d)
        if self._native_ok():
            return self._adapt_native(batch)
        try:
            return self._adapt_autograd(batch, image, gt_keypoints_2d)
        finally:
            from .fused_level import clear_last_forward
            clear_last_forward()                 # the remembered level forwards (and their activation arenas) end with the frame

    def _adapt_autograd(self, batch, image, gt_keypoints_2d):
        o = self.options
        if not o.use_boa:
            loss, _ = self.lower_level_adaptation(image, gt_keypoints_2d, None, self.model)
            self.optimizer.zero_grad(); loss.backward(); self.optimizer.step()
            return self.inference(batch, self.model)
        # Forward sharing (share_forwards=1): the reference's schedule evaluates several forwards whose weights AND
        # input are identical to a level forward of the same frame - the un-adapted feature forward (= lower level 0,
        # the learner being a fresh clone) and every inference() after an inner step (= the next level's forward with
        # the same fast weights).  Same kernels, same inputs => same bits, so those results are taken from the level
        # forwards: 9 HMR forwards per frame become 5 with every output of the reference schedule still produced.
        share = bool(getattr(o, "share_forwards", 1))
        if not share:
            def _feats():
                with torch.no_grad():
                    return self.model(image, need_feature=True)[3]
            init_features = self._on_side(_feats, image)
        elif o.inner_step == 0:
            # no lower level to share a forward with (the reference handles inner_step=0: dynaboa_benchmark.py:132-136)
            with torch.no_grad():
                init_features = [f.detach() for f in self.model(image, need_feature=True)[3]]
        h36m_batch = None
        learner = self.model.clone()
        owed = None                              # (tag, learner) of an inference() waiting for the next level forward
        for i in range(o.inner_step):
            lower_loss, lfeats = self.lower_level_adaptation(image, gt_keypoints_2d, h36m_batch, learner)
            if share and i == 0:
                init_features = [f.detach() for f in lfeats]
            if owed is not None:
                m, p, _ = self.inference(batch, learner, tag=owed, _pred=self._level_pred)
                self.mpjpe_all_lower[owed[1]].append(m); self.pampjpe_all_lower[owed[1]].append(p)
                owed = None
            if learner.first_order:
                learner.adapt(lower_loss)           # the reference's call (dynaboa_benchmark.py:140)
            else:
                learner.adapt(lower_loss, closure=self.level_closure("lower", image, gt_keypoints_2d, h36m_batch),
                              hvp_factory=self.level_hvp_factory("lower", image, gt_keypoints_2d, learner))
            if o.eval_lower:
                if share:
                    owed = ('lower', i)
                else:
                    m, p, _ = self.inference(batch, learner, tag=('lower', i))
                    self.mpjpe_all_lower[i].append(m); self.pampjpe_all_lower[i].append(p)
        upper_loss, _ = self.upper_level_adaptation(image, gt_keypoints_2d, h36m_batch, learner)
        if owed is not None:
            m, p, _ = self.inference(batch, learner, tag=owed, _pred=self._level_pred)
            self.mpjpe_all_lower[owed[1]].append(m); self.pampjpe_all_lower[owed[1]].append(p)
        self.optimizer.zero_grad()
        upper_loss.backward()
        self._join_side()                       # side-stream readers of theta must be done before the in-place step
        self.optimizer.step()
        if o.use_meanteacher:
            self.update_teacher(self.teacher, self.model)
        mpjpe, pampjpe, pve = self.inference(batch, self.model, tag=('final', 0))
        if self.global_step < len(self.mpjpe_statistics):
            self.mpjpe_statistics[self.global_step] = [mpjpe]
            self.pampjpe_statistics[self.global_step] = [pampjpe]
        if o.dynamic_boa:
            self._join_side()                   # init_features were produced on the side stream
            init_features = self._resolve(init_features)
            with torch.no_grad():
                adapted = self.model(image, need_feature=True)[3]
                sims = self.cal_feature_diff(init_features, adapted)
                feat_12 = float(sims[12]['cos'])
                self.feat_sims[self.global_step] = [sims]
            self.optimized_step = 0
            while 1 - feat_12 > o.cos_sim_threshold:
                self.optimized_step += 1
                if self.optimized_step > o.optim_steps:
                    break
                upper_loss, adapted = self.upper_level_adaptation(image, gt_keypoints_2d, h36m_batch, self.model)
                self.optimizer.zero_grad()
                upper_loss.backward()
                self._join_side()
                self.optimizer.step()
                if o.use_meanteacher:
                    self.update_teacher(self.teacher, self.model)
                with torch.no_grad():
                    init_features = [f.detach().clone() for f in adapted]
                    adapted = self.model(image, need_feature=True)[3]
                    sims = self.cal_feature_diff(init_features, adapted)
                    feat_12 = float(sims[12]['cos'])
                    self.feat_sims[self.global_step].append(sims)
                mpjpe, pampjpe, pve = self.inference(batch, self.model, tag=('final', self.optimized_step))
                # the reference appends the metrics of every extra step (dynaboa_benchmark.py:188-189: what it dumps to
                # steps_statistic_res.pt); in deferred mode the values live in metric_records under tag ('final', k)
                if mpjpe is not None and pampjpe is not None and self.global_step < len(self.mpjpe_statistics):
                    self.mpjpe_statistics[self.global_step].append(mpjpe)
                    self.pampjpe_statistics[self.global_step].append(pampjpe)
            self.optim_step_record.append(self.optimized_step)
        return mpjpe, pampjpe, pve

    # ------------------------------------------------------------------ metrics
    def _regress14(self, verts):
        lib = _lib.load()
        B = verts.shape[0]
        if not hasattr(self, "_Jh36m_dev"):
            self._Jh36m_dev = self.J_regressor.to(self.device).contiguous()
            # device-resident index: indexing with a Python list would build the index on the host and
            # do a synchronous H2D copy on every call (a full pipeline drain, 8x per frame)
            self._j14_idx = torch.tensor(self.joint_mapper_h36m, dtype=torch.long, device=self.device)
        out = torch.empty(B, 17, 3, device=self.device)
        v = verts.contiguous()
        check(lib.dyb_regress_joints(self._Jh36m_dev.data_ptr(), v.data_ptr(), out.data_ptr(), 17, B, stream_of(v)),
              "dyb_regress_joints")
        return out.index_select(1, self._j14_idx) - out[:, 0:1, :]

    def inference(self, batch, model, need_feature=False, tag=None, _step=None, _pred=None):
        """reference dynaboa_benchmark.py:204-262.  `_pred` = (rotmat, shape, cam) of a forward that already ran with
        exactly these weights on this image (adaptation() shares the level forwards, see there): the model call is
        skipped, everything downstream is the same code."""
        step = self.global_step if _step is None else _step
        if self._side is not None and self.options.deferred_metrics and not need_feature \
                and torch.cuda.current_stream(self.device) != self._side:
            reads = [self._theta_of(model)] + [v for v in batch.values() if torch.is_tensor(v)] + list(_pred or ())
            out = self._on_side(lambda: self.inference(batch, model, need_feature, tag, _step=step, _pred=_pred), *reads)
            return (None, None, None) if isinstance(out, dict) else out      # deferred: values come from flush_metrics()
        image, gt_pose, gt_betas, gender = batch['image'], batch['pose'], batch['betas'], batch['gender']
        model.eval()
        with torch.no_grad():
            if _pred is not None and not need_feature:
                out = _pred
            else:
                out = model(image, need_feature)
            pred_rotmat, pred_shape, pred_cam = out[0], out[1], out[2]
            smpl_out = self.decode_smpl_params(pred_rotmat, pred_shape)
            pred_vertices = smpl_out['vts']
            # the ground-truth side depends on the batch only: the 2-4 inference() calls of a frame share it
            key = (step, gt_pose.data_ptr(), gt_betas.data_ptr(), gender.data_ptr())
            cached = getattr(self, "_gt_cache", None)
            if cached is None or cached[0] != key:
                gt_vertices = self.smpl_male(global_orient=gt_pose[:, :3], body_pose=gt_pose[:, 3:], betas=gt_betas).vertices
                gt_female = self.smpl_female(global_orient=gt_pose[:, :3], body_pose=gt_pose[:, 3:], betas=gt_betas).vertices
                gt_vertices = torch.where((gender == 1).view(-1, 1, 1), gt_female, gt_vertices)
                gt_neutral = self.smpl_neutral(betas=gt_betas, body_pose=gt_pose[:, 3:], global_orient=gt_pose[:, :3],
                                               pose2rot=True).vertices
                cached = self._gt_cache = (key, self._regress14(gt_vertices), gt_neutral)
            gt14, gt_neutral = cached[1], cached[2]
            pred14 = self._regress14(pred_vertices)
            mpjpe_t = (pred14 - gt14).norm(dim=-1).mean(dim=-1)
            pve_t = (gt_neutral - pred_vertices).norm(dim=-1).mean()
        if self.options.dump_predictions:
            self.dump_prediction(pred_vertices, pred_cam, pred_rotmat, pred_shape)
        if getattr(self.options, "save_res", 0) and (tag is None or tag[0] == 'final'):
            # reference dynaboa_benchmark.py:257-258 (its call passes two arguments too many and would raise; the method's own
            # signature is used).  There every inference() of a frame writes Pred_{step}.png and the last one's file stays; here
            # only the inference() behind an optimiser step ('final'; no tag: a caller of its own) draws - the lower-level
            # evaluations of the same frame would only be overwritten
            self.save_results(pred_vertices, pred_cam, image, batch.get('imgname'), batch.get('bbox'), prefix='Pred')
        if self.options.deferred_metrics:
            self._pending.append(dict(step=step, tag=tag, pred=pred14, gt=gt14, mpjpe=mpjpe_t, pve=pve_t))
            res = (mpjpe_t, None, pve_t)
        else:
            pa = pa_mpjpe_device(pred14, gt14).cpu().numpy()
            res = (mpjpe_t.cpu().numpy() * 1000, pa * 1000, float(pve_t) * 1000)
        return res + (out[3],) if need_feature else res

    def flush_metrics(self):
        """Resolve deferred records: one Procrustes launch over every record, one device->host transfer of scalars."""
        return flush_metrics_of([self])[0]


_SYNC_ERRORS_SEEN = 0


def check_sync_errors():
    """The library's in-kernel hand-offs (one-pass GroupNorm backward: the workgroups of a slab meet on a counter) give up after ~0.2 s
    rather than block the queue, and the launch then goes on with incomplete sums.  Called where the host synchronises anyway (the
    metric flush): a non-zero count means adapted weights since the last check cannot be trusted - fail loudly."""
    import ctypes
    if not torch.cuda.is_available():
        return
    from . import _lib
    global _SYNC_ERRORS_SEEN
    n = ctypes.c_uint(0)
    rc = _lib.load().dyb_sync_error_count(ctypes.byref(n), torch.cuda.current_stream().cuda_stream)
    # the library's count is process-wide and monotonic: report only what is NEW since the last check, so one reported time-out does
    # not make every later flush of the process raise
    new, _SYNC_ERRORS_SEEN = n.value - _SYNC_ERRORS_SEEN, n.value
    if rc != 0 or new != 0:
        raise RuntimeError(f"libdynaboa_hip: {new} in-kernel hand-off(s) timed out since the last check (rc {rc}): results are invalid; "
                           "set DYB_TP_GN_ONEPASS=1 (single-workgroup slabs only) on a shared or partitioned GPU")


def final_selection(rec):
    """Indices of the records a frame's result is read from: the LAST 'final' record of every step (the dynamic loop appends one
    per extra step, directly behind each other)."""
    sel = []
    for i, r in enumerate(rec):
        if r['tag'] is not None and r['tag'][0] == 'final':
            prev = rec[i - 1] if i else None
            if sel and prev['step'] == r['step'] and prev['tag'] is not None and prev['tag'][0] == 'final':
                sel[-1] = i
            else:
                sel.append(i)
    return sel


SEQ_KEYS = ("accel", "accel_counted", "pck", "auc", "per_sequence")
_FRAME_ID = re.compile(r"image_(\d+)")


def _frame_ids(names, n):
    """The frames' numbers in their video from their imgname (3DPW: .../image_00042.jpg), or None unless all n names parse."""
    if names is None or len(names) != n:
        return None
    ids = [_FRAME_ID.search(str(x)) if x is not None else None for x in names]
    return None if any(m is None for m in ids) else [int(m.group(1)) for m in ids]


def _sequence_metrics_of(adaptors, recs):
    """--seq_metrics 1: the last final record of every step of every adaptor, step-major and then batch, through ONE dyb_seq_metrics
    call; every adaptor is one sequence unless it carries `_seq_lengths`.  -> (frame, seq, parts, lengths): the two device tensors,
    per adaptor (first frame, frames, first sequence row, names), all sequences' lengths - or None where there is no final record."""
    pred, gt, lengths, parts, ids, f0 = [], [], [], [], [], 0
    for k, (a, rec) in enumerate(zip(adaptors, recs)):
        sel = final_selection(rec)
        pred += [rec[i]['pred'] for i in sel]
        gt += [rec[i]['gt'] for i in sel]
        nf = sum(int(rec[i]['pred'].shape[0]) for i in sel)
        ln = getattr(a, "_seq_lengths", None) or [nf]
        if sum(ln) != nf:
            raise RuntimeError(f"--seq_metrics: sequence lengths {ln} for {nf} frame records")
        names = getattr(a, "_seq_names", None)
        if not names or len(names) != len(ln):
            base = getattr(getattr(a, "options", None), "expname", None) or "sequence"
            names = [base if len(ln) == 1 and len(adaptors) == 1 else f"{base}_{k}_{j}" for j in range(len(ln))]
        parts.append((f0, nf, len(lengths), list(names)))
        lengths += ln
        ids.append(_frame_ids(getattr(a, "_frame_names", None), nf))
        f0 += nf
    if not pred:
        return None
    pred, gt = torch.cat(pred), torch.cat(gt)
    fid = None if any(x is None for x in ids) else torch.tensor([v for x in ids for v in x], dtype=torch.int32)
    frame, seq = PU.sequence_metrics_device(pred, gt, lengths, frame_id=fid)
    return frame, seq, parts, lengths


def flush_metrics_of(adaptors):
    """`Adaptor.flush_metrics` for several adaptors at once (the sequences of a ReplicaGroup): the deferred records of all of them
    go through ONE Procrustes launch and ONE device->host transfer instead of one of each per adaptor.  -> list of the per-adaptor
    dicts `flush_metrics` returns.  With --seq_metrics 1 the same transfer also carries the output of one dyb_seq_metrics call and
    every dict gains SEQ_KEYS: accel (mm) / accel_counted / pck / auc per frame and per_sequence, a list of dicts (name, frames,
    mpjpe, pampjpe, pck, auc, accel, triples); the other keys and their values are what they are without the flag."""
    for a in adaptors:
        if a._native is not None:
            a._native.join()
        if a._side is not None:
            a._join_side()
            a._side.synchronize()
    recs = []
    for a in adaptors:
        recs.append(a._pending)
        a._pending = []
    flat = [r for rec in recs for r in rec]
    want_seq = bool(adaptors) and bool(getattr(getattr(adaptors[0], "options", None), "seq_metrics", 0))
    sm = None
    if flat:
        pred = torch.stack([r['pred'] for r in flat])
        gt = torch.stack([r['gt'] for r in flat])
        n, B = pred.shape[0], pred.shape[1]
        # Procrustes on the device: only scalars cross PCIe (one transfer for the whole run)
        pa_t = pa_mpjpe_device(pred.reshape(n * B, 14, 3), gt.reshape(n * B, 14, 3)).view(n, B)
        allm = torch.cat([torch.stack([r['mpjpe'] for r in flat]).reshape(n, B), pa_t,
                          torch.stack([r['pve'] for r in flat]).reshape(n, 1)], 1)
        sm = _sequence_metrics_of(adaptors, recs) if want_seq else None
        if sm is None:
            allm = allm.cpu().numpy() * 1000
        else:
            host = torch.cat([allm.flatten(), sm[0].flatten(), sm[1].flatten()]).cpu().numpy()
            k0, k1 = allm.numel(), allm.numel() + sm[0].numel()
            allm = host[:k0].reshape(n, 2 * B + 1) * 1000
            frame, seqrows = host[k0:k1].reshape(-1, PU.FRAME_FLOATS), host[k1:].reshape(-1, PU.SEQ_FLOATS)
    check_sync_errors()
    outs, i0 = [], 0
    for k, rec in enumerate(recs):
        out = dict(mpjpe=[], pampjpe=[], pve=[], records=[])
        if rec:
            m = allm[i0:i0 + len(rec)]
            i0 += len(rec)
            mp, pa, pve = m[:, :B], m[:, B:2 * B], m[:, 2 * B]
            for i, r in enumerate(rec):
                out['records'].append(dict(step=r['step'], tag=r['tag'], mpjpe=mp[i], pampjpe=pa[i], pve=float(pve[i])))
            for i in final_selection(rec):
                out['mpjpe'].append(mp[i]); out['pampjpe'].append(pa[i]); out['pve'].append(float(pve[i]))
        if want_seq:
            out.update(accel=np.zeros(0, np.float32), accel_counted=np.zeros(0, bool), pck=np.zeros(0, np.float32),
                       auc=np.zeros(0, np.float32), per_sequence=[])
            if sm is not None:
                f0, nf, s0, names = sm[2][k]
                f = frame[f0:f0 + nf]
                out.update(accel=f[:, PU.FRAME_ACCEL] * 1000, accel_counted=f[:, PU.FRAME_ACCEL_COUNTED] > 0.5,
                           pck=f[:, PU.FRAME_PCK].copy(), auc=f[:, PU.FRAME_AUC].copy(),
                           per_sequence=[sequence_row(nm, seqrows[s0 + j]) for j, nm in enumerate(names)])
        outs.append(out)
    return outs


def sequence_row(name, row):
    """One row of dyb_seq_metrics' per-sequence output (metres) as the report's dict (mm)."""
    return dict(name=str(name), frames=int(row[PU.SEQ_FRAMES]), mpjpe=float(row[PU.SEQ_MPJPE]) * 1000,
                pampjpe=float(row[PU.SEQ_PAMPJPE]) * 1000, pck=float(row[PU.SEQ_PCK]), auc=float(row[PU.SEQ_AUC]),
                accel=float(row[PU.SEQ_ACCEL]) * 1000, triples=int(row[PU.SEQ_TRIPLES]))


def sequence_summary(res):
    """-> (overall, sequence_mean) of a result dict with SEQ_KEYS: the frame-weighted means over all frames (the acceleration error
    over the counted triples) and the unweighted means over the sequences that have frames (accel: that have a triple)."""
    flat = lambda x: np.ravel(x).astype(np.float64) if isinstance(x, np.ndarray) else \
        np.concatenate([np.ravel(np.asarray(v, np.float64)) for v in x]) if len(x) else np.zeros(0)
    mean = lambda v: float(np.mean(v)) if len(v) else 0.0
    counted = np.asarray(res["accel_counted"], bool)
    overall = dict(frames=int(len(res["pck"])), mpjpe=mean(flat(res["mpjpe"])), pampjpe=mean(flat(res["pampjpe"])),
                   pve=mean(np.ravel(np.asarray(res["pve"], np.float64))), pck=mean(np.asarray(res["pck"], np.float64)),
                   auc=mean(np.asarray(res["auc"], np.float64)), accel=mean(np.asarray(res["accel"], np.float64)[counted]),
                   triples=int(counted.sum()))
    rows = [r for r in res["per_sequence"] if r["frames"] > 0]
    seq_mean = {k: mean([r[k] for r in rows]) for k in ("mpjpe", "pampjpe", "pck", "auc")}
    seq_mean["accel"] = mean([r["accel"] for r in rows if r["triples"] > 0])
    return overall, seq_mean


def write_sequence_report(exppath, options, res):
    """<exppath>/metrics.json (overall frame-weighted means, the mean over sequences, the flags of the run) and
    <exppath>/metrics_per_sequence.csv (one line per sequence, worst PA-MPJPE first)."""
    import json
    os.makedirs(exppath, exist_ok=True)
    overall, seq_mean = sequence_summary(res)
    flags = {k: v for k, v in sorted(vars(options).items()) if isinstance(v, (int, float, str, bool, type(None)))}
    with open(os.path.join(exppath, "metrics.json"), "w") as f:
        json.dump(dict(overall=overall, sequence_mean=seq_mean, sequences=len(res["per_sequence"]), flags=flags), f, indent=1)
    cols = ("name", "frames", "mpjpe", "pampjpe", "pck", "auc", "accel", "triples")
    with open(os.path.join(exppath, "metrics_per_sequence.csv"), "w") as f:
        f.write(",".join(cols) + "\n")
        for r in sorted(res["per_sequence"], key=lambda r: -r["pampjpe"]):
            f.write(",".join(str(r[c]) for c in cols) + "\n")
    return overall, seq_mean


def sequence_line(res):
    overall, _ = sequence_summary(res)
    return f"ACCEL:{overall['accel']}, PCK:{overall['pck']}, AUC:{overall['auc']}"


if __name__ == '__main__':
    options = parser.parse_args()
    if options.num_shards > 1 or options.seqs_per_gpu > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
        from dynaboa_amd import sharded
        sharded.main(options)
    else:
        adaptor = Adaptor(options)
        res = adaptor.excute()
        print(f"MPJPE:{np.mean(res['mpjpe'])}, PAMPJPE:{np.mean(res['pampjpe'])}, PVE:{np.mean(res['pve'])}")
        if options.seq_metrics:
            print(sequence_line(res))
