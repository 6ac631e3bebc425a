"""In-the-wild ("internet") videos: AlphaPose detections -> dataset -> adaptation, the reference's ``--dataset internet`` path
(``utils/data_preprocess/internet_data.py``, ``boa_dataset/internet_data.py``, ``dynaboa_internet.py``).

    python -m dynaboa_amd.internet --extract DIR        # every DIR/<seq>.json (AlphaPose records) -> DIR/<seq>.npz
    python -m dynaboa_amd.internet --internet_root DIR [--save_res 1] [--native_results 0]
                                   [--split_tracks 1 --min_track_frames N --seqs_per_gpu S --num_shards N]
                                   [--scene_overlays 1 | --compose_only 1]

The second form is the reference's ``dynaboa_internet.py`` with its flags and defaults: adaptation, then one inference per row, no
metrics; it writes ``<expdir>/<expname>/result/Pred_{n}.pt`` (``verts``, ``cam``, ``rotmat``, ``beta``) for every row and, with
``--save_res 1``, the overlay ``image/Pred_{n}.png``.  n is the row's index in the concatenated npz order - the reference's
``global_step`` in the default single stream, and unique over tracks under ``--split_tracks``.  ``--native_results`` defaults to 1
in this driver: the run stays on the native frame stepper and the files come from its result ring; 0 runs the autograd composition.

A folder of an internet video holds ``<seq>.json`` (one record per detected person and frame: ``image_id``, ``keypoints`` 17 x 3
COCO joints, ``score``, ``idx``), the frames under ``images/<seq>/`` and, after ``--extract``, ``<seq>.npz`` with ``imgname``,
``center``, ``scale``, ``part`` as the reference writes them plus one array the reference does not have: ``track``, the detection's
``idx[0]`` as an integer (-1 when absent) - the reference's loader ignores unknown keys, so the files stay readable by it.

What differs from the reference, on purpose:
  * the npz files are read in sorted order (the reference walks an unsorted ``glob``: its row order depends on the file system);
  * the stored keypoints are never modified (the reference's ``j2d_processing`` writes the transformed coordinates back into the
    loaded array through a view, so a row read twice comes out different the second time);
  * several people of one video can be adapted as separate sequences: ``split_tracks`` makes one sequence per (file, track) instead of
    the reference's single stream over all people interleaved, whose motion term compares a person with whoever stood ``interval``
    rows earlier.  A lockstep step of such sequences cuts all its crops with one ``datasets.preprocess_frames`` call, and a frame
    that two tracks share is decoded and uploaded once;
  * ``--scene_overlays 1`` draws, after the adaptation, ONE picture per video frame with every adapted person of that frame in it
    (``scene/<seq>/<frame>.png``; ``compose_scenes``) - the reference has one picture per person.  ``--compose_only 1`` runs just
    that pass over the ``result/Pred_{n}.pt`` files of an existing experiment directory (after a sharded run, for one)."""
from __future__ import annotations

import argparse
import copy
import glob
import json
import os
import re
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import benchmark as DB
from . import constants as C
from . import datasets as D
from .jpeg import sink_for

INTERNET_ROOT = "data/internet_data"             # stands for the reference's config.InternetData_ROOT (--internet_root)
MIN_SCORE, MIN_HEIGHT, CONF_THRESHOLD = 2.5, 250, 0.3
# slot of each COCO-17 joint (nose, l/r eye, l/r ear, l/r shoulder, l/r elbow, l/r wrist, l/r hip, l/r knee, l/r ankle) in the
# 49-joint layout (constants.JOINT_NAMES): all of them in 25..48, the window of keypoint set "gt24"
COCO_TO_49 = (44, 45, 46, 47, 48, 34, 33, 35, 32, 36, 31, 28, 27, 29, 26, 30, 25)


def synthetic_frame(step: int, seed: int = 22) -> Dict[str, object]:
    """A seeded synthetic batch of one frame in the item schema (assets.make_frame's image and keypoints), its keypoints COCO-shaped:
    the 17 mapped joints of the 49 keep position and confidence, every other row - the 25 OpenPose slots and the 7 unmapped joints
    of the gt24 window - is exactly zero.  What the stream goldens (tools/make_golden_internet.py) and their tests run on."""
    from . import assets
    fr = assets.make_frame(step, 1, seed=seed)
    kp = torch.zeros_like(fr["smpl_j2d"])
    kp[:, list(COCO_TO_49)] = fr["smpl_j2d"][:, list(COCO_TO_49)]
    return dict(image=fr["image"], smpl_j2d=kp, imgname=[f"synthetic/{step:06d}.png"], bbox=torch.tensor([[112.0, 112.0, 224.0]], dtype=torch.float64),
                row=[step])


# ---------------------------------------------------------------------------------------- detections -> npz
def person_height(j2d: np.ndarray) -> float:
    """Norm of the extent of the joints with confidence > 0.3 (internet_data.py:35-40).  A detection without such a joint has no
    extent: 0 here, so it is dropped (the reference would stop on the empty reduction)."""
    vis = j2d[:, 2] > CONF_THRESHOLD
    if not vis.any():
        return 0.0
    return float(np.linalg.norm(np.max(j2d[vis, :2], 0) - np.min(j2d[vis, :2], 0)))


def detection_bbox(j2d: np.ndarray):
    """Centre and scale from the min / max of ALL 17 joints, whatever their confidence (internet_data.py:28-33)."""
    x0, y0, x1, y1 = min(j2d[:, 0]), min(j2d[:, 1]), max(j2d[:, 0]), max(j2d[:, 1])
    return [(x1 + x0) / 2, (y1 + y0) / 2], 1. * max(x1 - x0, y1 - y0) / 200


def track_of(annot: dict) -> int:
    idx = annot.get("idx", None)
    if isinstance(idx, (list, tuple)):
        idx = idx[0] if idx else None
    return -1 if idx is None else int(idx)


def internet_data_extract(in_path: str, track: int = 0, device="cuda", **rule) -> List[str]:
    """reference utils/data_preprocess/internet_data.py:42-79: for every ``<seq>.json`` of `in_path` (in name order) keep the
    detections with score >= 2.5 and person height >= 250 and write ``<seq>.npz``.  track = 1 (--track 1): the ``track`` array comes
    from ``tracked_ids`` instead of the records' ``idx``.  -> the files written."""
    seqs = sorted(os.path.basename(n)[:-5] for n in glob.glob(os.path.join(in_path, '*.json')))
    written, pending = [], []
    for seq in seqs:
        with open(os.path.join(in_path, f'{seq}.json')) as fh:
            annots = json.load(fh)
        imagenames, scales, centers, j2ds, tracks, raw = [], [], [], [], [], []
        for annot in annots:
            kps2d = np.array(annot['keypoints']).reshape(-1, 3)
            if annot['score'] < MIN_SCORE or person_height(kps2d) < MIN_HEIGHT:
                continue
            if kps2d.shape != (17, 3):
                raise ValueError(f"{seq}.json: a detection with {kps2d.shape[0]} joints (COCO-17 expected)")
            center, scale = detection_bbox(kps2d)
            if track:
                raw.append(kps2d.astype(np.float32))                    # the raw confidences, before the 0 / 1 rewrite
            kps2d[:, 2] = kps2d[:, 2] > CONF_THRESHOLD
            part = np.zeros([C.NUM_OUT_JOINTS, 3])
            part[list(COCO_TO_49)] = kps2d
            imagenames.append(os.path.join(seq, annot['image_id']))
            centers.append(center); scales.append(scale); j2ds.append(part); tracks.append(track_of(annot))
        arrays = dict(imgname=imagenames, center=centers, scale=scales, part=j2ds, track=np.array(tracks, dtype=np.int64))
        if track:
            pending.append((seq, len(annots), arrays, raw))              # written below, after the one call over all files
        else:
            written.append(_write_extract(in_path, seq, len(annots), arrays))
    if track:
        for (_, _, arrays, _), ids in zip(pending, tracked_ids([(p[2]["imgname"], p[3]) for p in pending], device=device, **rule)):
            arrays["track"] = ids
        written = [_write_extract(in_path, seq, total, arrays) for seq, total, arrays, _ in pending]
    return written


def _write_extract(in_path, seq, total, arrays):
    out_file = os.path.join(in_path, f'{seq}.npz')
    np.savez(out_file, **arrays)
    print(f'{seq}: {total} detections, {len(arrays["imgname"])} kept')
    return out_file


def tracked_ids(videos, device="cuda", **rule) -> List[np.ndarray]:
    """--extract --track 1.  videos: per file (image names, raw (17, 3) detections) of the rows it keeps, in record order.  A video's
    frames are its distinct image names in order of first appearance, numbered by the trailing digits of their stems when all of
    them parse and increase (else by position); ALL videos go into one ``track.track_videos`` call.  -> per file the rows' ids
    (int64; -1: a detection the rule leaves without a track)."""
    from . import track as T
    batch, ids, where = [], [], []
    for names, raw in videos:
        frames: Dict[str, List[int]] = {}
        for row, name in enumerate(names):
            frames.setdefault(name, []).append(row)                       # dicts keep first-appearance order
        order, rows_of = list(frames), list(frames.values())
        num = [re.search(r"(\d+)$", os.path.splitext(os.path.basename(n))[0]) for n in order]
        fid = None
        if all(m is not None for m in num) and len({int(m.group(1)) for m in num}) == len(num):
            by_id = sorted(range(len(order)), key=lambda i: int(num[i].group(1)))     # records out of frame order: the numbers decide
            rows_of, fid = [rows_of[i] for i in by_id], [int(num[i].group(1)) for i in by_id]
        batch.append([np.stack([raw[r] for r in rows]) for rows in rows_of])
        ids.append(fid)
        where.append(rows_of)
    if any(x is None for x in ids):
        ids = None
    tracks, _, _ = T.track_videos(batch, ids, device=device, **rule)
    out = []
    for (names, _), rows_of, per_frame in zip(videos, where, tracks):
        col = -np.ones(len(names), np.int64)
        for rows, tr in zip(rows_of, per_frame):
            col[rows] = tr
        out.append(col)
    return out


# ---------------------------------------------------------------------------------------- dataset
class InternetDataset:
    """reference ``Internet_dataset`` (boa_dataset/internet_data.py:16-97): every row of every ``<root>/*.npz``, the files in sorted
    order (the reference: unsorted glob).  An item is the reference's - ``image`` (3, 224, 224) normalised crop, ``imgname``,
    ``smpl_j2d`` (49, 3) keypoints in the crop frame in [-1, 1], ``bbox`` = [cx, cy, 200 * scale] - plus ``row``, the row's index in the
    concatenated file order (what ``Pred_{n}`` is numbered by).  The stored keypoints stay as loaded: the reference's in-place
    rewrite of them (its ``j2d_processing`` transforms a view of the array) is NOT reproduced.

    ``sequences``: one stream over all rows in file order by default (the reference's behaviour, the parity mode); with
    ``split_tracks`` one sequence per (file, track) with at least ``min_track_frames`` rows, in order of first appearance - the rows
    without a track (-1) of a file are one such sequence.  A sequence is ``dict(file, track, first, frames, rows)``; ``rows`` lists its
    row indices (those of a track are not contiguous)."""

    def __init__(self, options=None, root: Optional[str] = None, device="cuda", files: Optional[Sequence[str]] = None,
                 split_tracks: Optional[int] = None, min_track_frames: Optional[int] = None):
        root = root or getattr(options, "internet_root", None) or INTERNET_ROOT
        self.options, self.root, self.img_dir, self.device = options, root, os.path.join(root, 'images'), torch.device(device)
        self.files = sorted(files if files is not None else glob.glob(os.path.join(root, '*.npz')))
        self.split_tracks = int(getattr(options, "split_tracks", 0) if split_tracks is None else split_tracks)
        self.min_track_frames = int(getattr(options, "min_track_frames", 1) if min_track_frames is None else min_track_frames)
        names, scales, centers, parts, tracks, file_of = [], [], [], [], [], []
        for fi, f in enumerate(self.files):
            d = np.load(f)
            n = int(d['scale'].shape[0])
            if n == 0:
                continue
            names.append(d['imgname']); scales.append(d['scale']); centers.append(d['center']); parts.append(d['part'])
            tracks.append(d['track'].astype(np.int64) if 'track' in d.files else -np.ones(n, np.int64))
            file_of.append(np.full(n, fi, np.int64))
        cat = lambda v, empty: np.concatenate(v, 0) if v else empty
        self.imgnames, self.scales = cat(names, np.zeros((0,), dtype=str)), cat(scales, np.zeros((0,)))
        self.centers, self.smpl_j2ds = cat(centers, np.zeros((0, 2))), cat(parts, np.zeros((0, C.NUM_OUT_JOINTS, 3)))
        self.tracks, self.file_of = cat(tracks, np.zeros((0,), np.int64)), cat(file_of, np.zeros((0,), np.int64))
        self.smpl_j2ds.setflags(write=False)
        self.sequences = self._sequences()

    def _sequences(self) -> List[dict]:
        n = len(self)
        if not self.split_tracks:
            return [dict(file=None, track=None, first=0, frames=n, rows=list(range(n)))] if n else []
        groups: Dict[tuple, List[int]] = {}
        for i in range(n):
            groups.setdefault((int(self.file_of[i]), int(self.tracks[i])), []).append(i)      # dicts keep first-appearance order
        return [dict(file=self.files[fi], track=tr, first=rows[0], frames=len(rows), rows=rows)
                for (fi, tr), rows in groups.items() if len(rows) >= self.min_track_frames]

    def __len__(self):
        return int(self.scales.shape[0])

    def read_frame(self, imgname: str) -> np.ndarray:
        return D.read_image(os.path.join(self.img_dir, imgname))

    def annotations(self, index: int) -> dict:
        """The host half of an item without its frame."""
        scale, center = float(self.scales[index]), np.array(self.centers[index], dtype=np.float64)
        return dict(scale=scale, center=center, imgname=str(self.imgnames[index]), row=int(index),
                    smpl_j2d=D.j2d_processing(self.smpl_j2ds[index], center, scale))

    def host_item(self, index: int) -> dict:
        h = self.annotations(index)
        h["frame"] = self.read_frame(h["imgname"])
        return h

    def device_annotations(self, h: dict, image: torch.Tensor) -> dict:
        dev = self.device
        return dict(image=image, imgname=h["imgname"], smpl_j2d=torch.from_numpy(h["smpl_j2d"]).to(dev, non_blocking=True),
                    bbox=torch.tensor([h["center"][0], h["center"][1], h["scale"] * 200], dtype=torch.float64, device=dev), row=h["row"])

    def device_item(self, h: dict) -> dict:
        frame = torch.from_numpy(h["frame"]).to(self.device, non_blocking=True)
        return self.device_annotations(h, D.preprocess_frame(frame, h["center"], h["scale"]))

    def __getitem__(self, index: int) -> dict:
        return self.device_item(self.host_item(index))


class TrackGroupLoader:
    """The lockstep walk of several sequences of an InternetDataset: step t yields ``[(s, batch), ...]`` for every sequence s (index
    into `sequences`) that still has a row at t - a sequence that ends early leaves the list -, each batch a batch of one frame with
    the keys of ``datasets.collate``.  Per step every distinct frame is decoded and uploaded ONCE, however many sequences show a
    person on it, and all crops of the step are cut by one ``datasets.preprocess_frames`` call (``batched=False``: one
    ``preprocess_frame`` call per crop, the same bits - the comparison arm of tools/internet_rate.py).  Decoding runs `prefetch` steps
    ahead on `workers` threads."""

    def __init__(self, dataset: InternetDataset, sequences: Sequence[dict], workers: int = 8, prefetch: int = 4, batched: bool = True):
        self.ds, self.seqs, self.workers, self.prefetch, self.batched = dataset, list(sequences), workers, prefetch, batched
        self.decoded = 0                             # frames decoded so far (a shared frame counts once)

    def __len__(self):
        return max((len(s["rows"]) for s in self.seqs), default=0)

    def _host_step(self, t: int, pool):
        active = [(si, s["rows"][t]) for si, s in enumerate(self.seqs) if t < len(s["rows"])]
        ann = [self.ds.annotations(row) for _, row in active]
        frames = {}
        for a in ann:
            if a["imgname"] not in frames:
                frames[a["imgname"]] = pool.submit(self.ds.read_frame, a["imgname"])
        self.decoded += len(frames)
        return active, ann, frames

    def __iter__(self):
        ds, dev = self.ds, self.ds.device
        with ThreadPoolExecutor(max_workers=max(1, self.workers)) as pool:
            pending, nxt, T = [], 0, len(self)
            while nxt < T or pending:
                while nxt < T and len(pending) < self.prefetch:
                    pending.append(self._host_step(nxt, pool))
                    nxt += 1
                active, ann, frames = pending.pop(0)
                on_dev = {k: torch.from_numpy(f.result()).to(dev, non_blocking=True) for k, f in frames.items()}
                if self.batched:
                    images = D.preprocess_frames([on_dev[a["imgname"]] for a in ann], [a["center"] for a in ann], [a["scale"] for a in ann])
                else:
                    images = [D.preprocess_frame(on_dev[a["imgname"]], a["center"], a["scale"]) for a in ann]
                # keypoints and boxes of the whole step in one upload each; a track's batch is a slice of them
                kp = torch.from_numpy(np.stack([a["smpl_j2d"] for a in ann])).to(dev, non_blocking=True)
                bbox = torch.from_numpy(np.array([[a["center"][0], a["center"][1], a["scale"] * 200] for a in ann], dtype=np.float64)).to(dev, non_blocking=True)
                yield [(si, dict(image=images[i:i + 1] if self.batched else images[i].unsqueeze(0), imgname=[a["imgname"]],
                                 smpl_j2d=kp[i:i + 1], bbox=bbox[i:i + 1], row=[a["row"]]))
                       for i, ((si, _), a) in enumerate(zip(active, ann))]


# ---------------------------------------------------------------------------------------- adaptation
def _make_parser():
    """The flags and defaults of the reference's dynaboa_internet.py:16-65 - the same set as dynaboa_benchmark.py, so the
    benchmark driver's parser is copied, with this project's additions it already carries (--native_results, --seqs_per_gpu,
    --num_shards, ...) - plus the internet path's own.  --dataset defaults to internet and --dump_predictions to 1 here:
    ``result/Pred_{n}.pt`` is this driver's only product - and --native_results to 1, so that the dumps do not take the plain
    command off the native stepper (``native_step.coverage``); --native_results 0 runs the autograd composition."""
    p = copy.deepcopy(DB.parser)            # (a copy: `parents=` would share the argument objects, and set_defaults below would
    p.description = __doc__                 #  change the benchmark driver's own defaults with them)
    p.formatter_class = argparse.RawDescriptionHelpFormatter
    p.add_argument('--extract', type=str, default=None, metavar='DIR', help='write DIR/<seq>.npz for every DIR/<seq>.json and stop')
    p.add_argument('--track', type=int, default=0, choices=[0, 1],
                   help="--extract: 1: the track array of every <seq>.npz comes from the device tracker (dynaboa_amd.track: one call "
                        "over all files, on the detections that pass the score and height filters, with their raw confidences) instead "
                        "of the records' idx - for AlphaPose output without pose tracking; --c_min ... --min_common set the rule")
    from .track import add_rule_arguments
    add_rule_arguments(p)
    p.add_argument('--internet_root', type=str, default=INTERNET_ROOT, help="folder of the <seq>.npz files and images/ (the reference's "
                                                                           'config.InternetData_ROOT)')
    p.add_argument('--split_tracks', type=int, default=0, choices=[0, 1],
                   help="0: one stream over all rows in file order (the reference); 1: one sequence per (file, track)")
    p.add_argument('--min_track_frames', type=int, default=1, help='--split_tracks 1: drop tracks with fewer rows')
    p.add_argument('--scene_overlays', type=int, default=0, choices=[0, 1],
                   help='1: after the adaptation draw every frame once with all its adapted people: scene/<seq>/<frame>.png')
    p.add_argument('--compose_only', type=int, default=0, choices=[0, 1],
                   help='1: no adaptation - only the --scene_overlays pass over the result/Pred_{n}.pt of <expdir>/<expname>')
    p.add_argument('--smooth_window', type=int, default=0, metavar='H',
                   help='H > 0: after the adaptation (and with --compose_only 1) smooth every sequence of the dataset over 2 H + 1 frames '
                        '(dynaboa_amd.smooth.smooth_results): result_smooth/Pred_{n}.pt, and with --scene_overlays 1 scene_smooth/...; '
                        'a sequence is what the adaptation streams as one - with several people in a video pass --split_tracks 1')
    p.add_argument('--smooth_sigma', type=float, default=None, help='--smooth_window: sigma of the Gaussian weights in frames (default H / 2)')
    p.set_defaults(dataset='internet', dump_predictions=1, native_results=1)
    return p


parser = _make_parser()


def refuse_seq_metrics(options):
    """--seq_metrics comes with the benchmark driver's parser, but an internet video has no 3-D ground truth to measure against."""
    if getattr(options, "seq_metrics", 0):
        raise ValueError("--seq_metrics 1 needs 3-D ground truth (MPJPE, PCK / AUC and the acceleration error are errors against it): "
                         "internet videos have none - run it with --dataset 3dpw through dynaboa_amd.benchmark")


class Adaptor(DB.Adaptor):
    """reference dynaboa_internet.py:69-164: per frame adaptation (the benchmark's schedule: lower levels, upper level, teacher,
    dynamic loop) and then ONE inference without ground truth - no metrics; its products are ``result/Pred_{n}.pt`` (``verts``,
    ``cam`` in the cam_t form, ``rotmat``, ``beta``) and, with ``--save_res 1``, the overlay ``image/Pred_{n}.png``.  On the
    native stepper (``--native_results 1``) the stepper runs with ``metrics`` 0 and NULL ground truth, and both files are written
    from its result ring; otherwise from the last inference of the autograd composition.  One difference in the flag set: the
    reference's internet adaptation always runs the bilevel schedule and ignores ``--use_boa``; here ``--use_boa 0`` takes the
    benchmark driver's branch (one loss, one Adam step, on the autograd path)."""

    def __init__(self, options, assets_bundle=None, device=None):
        refuse_seq_metrics(options)
        options = copy.copy(options)          # the switches below are this adaptor's, not the caller's namespace's
        options.dataset = 'internet'
        options.metrics, options.eval_lower, options.deferred_metrics, options.overlap_metrics = 0, 0, 1, 0
        super().__init__(options, assets_bundle, device)
        self._last_pred = None

    def set_dataloader(self):
        """The stream is the InternetDataset also with a synthetic bundle (which only stands for checkpoint / SMPL / prior files)."""
        ds = self.dataset = InternetDataset(self.options, device=self.device)
        self.imgdir = ds.img_dir
        self.dataloader = D.FrameLoader(ds, batch_size=self.options.batch_size, workers=8) if len(ds) else None

    def inference(self, batch, model, need_feature=False, tag=None, _step=None, _pred=None):
        """No ground truth: an inference is the forward alone; the one behind the frame's last optimiser step is the result."""
        with torch.no_grad():
            out = _pred if (_pred is not None and not need_feature) else model(batch["image"], need_feature)
        if tag is None or tag[0] == "final":
            self._last_pred = (out[0].detach(), out[1].detach(), out[2].detach())
        res = (None, None, None)
        return res + (out[3],) if need_feature else res

    def _native_records(self, slot, nfinal):
        return (None, None, None)             # metrics = 0: the stepper writes no records

    def write_frame_results(self, batch):
        """Autograd path: Pred_{n}.pt / Pred_{n}.png of the frame's last inference (the native path wrote them from the ring)."""
        if self._last_pred is None:
            return
        rot, shape, cam = self._last_pred
        self._last_pred = None
        if not (self.options.dump_predictions or self.options.save_res):
            return
        with torch.no_grad():
            vts = self.decode_smpl_params(rot, shape)["vts"]
        if self.options.dump_predictions:
            self.dump_prediction(vts, cam, rot, shape)
        if self.options.save_res:
            self.save_results(vts, cam, batch["image"], batch.get("imgname"), batch.get("bbox"), prefix="Pred")

    def excute(self, frames=None, nframes=None):
        """reference dynaboa_internet.py:70-86.  `frames`: batches of the item schema (default: the whole dataset as one stream);
        a batch's ``row`` numbers its result files when the caller set ``number_by_row`` (--split_tracks: unique over tracks),
        else the step does, as in the reference."""
        frames = self.dataloader if frames is None else frames
        nframes = len(frames) if nframes is None else nframes
        self.reset_records(nframes)
        os.makedirs(os.path.join(self.exppath, 'result'), exist_ok=True)
        for step, batch in enumerate(frames):
            self.global_step = step
            self._result_step = int(batch["row"][0]) if getattr(self, "number_by_row", False) else None
            self.fit_losses = {}
            batch = {k: v.to(self.device) if isinstance(v, torch.Tensor) else v for k, v in batch.items()}
            self.model.eval()
            self.adaptation(batch)
            self.write_frame_results(batch)
            self.write_summaries(self.fit_losses)
        if self._native is not None:
            self._native.join()
        return None


def run_tracks(options, dataset: InternetDataset, make_adaptor, num_shards: int = 1, shard_rank: int = 0, seqs_per_gpu: int = 1,
               batched: bool = True) -> List[int]:
    """The metric-free counterpart of ``sharded.run_sharded`` for the sequences of an InternetDataset: the same assignment of whole
    sequences to ranks, the same waves of `seqs_per_gpu` (longest first) stepped in lockstep as replicas, the same ``set_active``
    handling of unequal lengths (a track that ends leaves the launch set) and the same numbering (result files carry the row's
    global index) - nothing is gathered, every rank writes its own rows' files.  make_adaptor() -> a fresh Adaptor at the base
    checkpoint.  -> the rows this rank adapted, in the order it finished them."""
    from . import native_step as NS
    from .base_adaptor import close_overlays
    from .sharding import assign_sequences
    seqs = dataset.sequences
    if int(getattr(options, "batch_size", 1)) != 1:
        raise ValueError("sequences of an internet video are adapted with batch_size 1")
    owned = assign_sequences([s["frames"] for s in seqs], num_shards)[shard_rank] if seqs else []
    order = sorted(owned, key=lambda i: (-seqs[i]["frames"], i))
    S = max(1, int(seqs_per_gpu))
    if S > 1 and not getattr(options, "native_results", 0):
        raise ValueError("--seqs_per_gpu > 1 writes its results from the native stepper's ring: pass --native_results 1")
    done: List[int] = []
    for w0 in range(0, len(order), S):
        wave = [seqs[i] for i in order[w0:w0 + S]]
        steps = max(s["frames"] for s in wave)
        ads = [make_adaptor() for _ in wave]
        for a, s in zip(ads, wave):                       # --overlay_video 1: one video per (file, track), video/Pred_<name>.avi
            if s.get("file") is not None:
                a.sequence_name = f"{os.path.splitext(os.path.basename(str(s['file'])))[0]}_track{s['track']}"
        if len(wave) == 1:
            ads[0].number_by_row = True
            ads[0].excute(D.FrameLoader(dataset, batch_size=1, workers=4, indices=wave[0]["rows"]), nframes=steps)
            done += list(wave[0]["rows"])
        else:
            grp = NS.ReplicaGroup(ads, steps)
            try:
                for step, items in enumerate(TrackGroupLoader(dataset, wave, workers=4, batched=batched)):
                    batches, numbers = [None] * len(wave), [0] * len(wave)
                    for si, b in items:
                        batches[si], numbers[si] = b, int(b["row"][0])
                    grp.step(batches, step, result_steps=numbers)
                    done += [numbers[si] for si, _ in items]
            finally:
                close_overlays(ads)                       # the tracks' videos stay open across the wave's steps and end with it
            grp.stepper.join()
        del ads
    return done


# ---------------------------------------------------------------------------------------- all people of a frame in one picture
SCENE_BATCH = 8              # frames drawn per scene call (a 1920 x 1080 frame and its picture are 6 MB each on the device)


def scene_path(exppath: str, imgname: str, out_dir: str = 'scene') -> str:
    """``<exppath>/scene/<seq>/<frame file stem>.png`` for the frame ``<seq>/<file>``."""
    return os.path.join(exppath, out_dir, os.path.splitext(imgname)[0] + '.png')


def scene_meshes(dataset: InternetDataset, exppath: str, rows: Sequence[int], width: int, height: int, result_dir: str = 'result'):
    """The adapted people of ONE frame (`rows`: its rows) as ``Renderer.render_scenes`` takes them, in painter order: [(verts
    (6890, 3) fp32, cam (4,) = (sx, sy, tx, ty) fp32 in the frame, colour)] from ``result/Pred_{n}.pt`` - the crop camera recovered
    from the stored ``cam_t`` (``render.parse_cam``), carried to the frame with the row's box (``convert_crop_cam_to_orig_img``), both
    in float64 and rounded once.  Every person has a camera of their own, so their depths cannot be compared: the order is by
    apparent size instead - ascending frame scale sx (the apparently smaller person goes underneath), then track id, then row.
    result_dir: the folder of the dumps (``result_smooth``: the smoothing pass's); a dump that carries ``cam_frame`` - the smoothed
    frame camera - is drawn under it instead."""
    import joblib
    from .render import convert_crop_cam_to_orig_img, parse_cam, track_color
    people = []
    for n in rows:
        path = os.path.join(exppath, result_dir, f'Pred_{n}.pt')
        if not os.path.isfile(path):
            raise FileNotFoundError(f"scene overlays: row {n} ({dataset.imgnames[n]}, track {int(dataset.tracks[n])}) has no {path}")
        d = joblib.load(path)
        cam = parse_cam(np.asarray(d['cam'], np.float64).reshape(1, 3))
        bbox = np.array([[dataset.centers[n][0], dataset.centers[n][1], float(dataset.scales[n]) * 200]], np.float64)
        ocam = convert_crop_cam_to_orig_img(cam, bbox, width, height)[0].astype(np.float32)
        if 'cam_frame' in d:
            ocam = np.asarray(d['cam_frame'], np.float32).reshape(4)
        people.append((float(ocam[0]), int(dataset.tracks[n]), int(n), np.asarray(d['verts'], np.float32).reshape(-1, 3), ocam))
    people.sort(key=lambda p: p[:3])
    return [(v, ocam, track_color(tr)) for _, tr, _, v, ocam in people]


def compose_scenes(dataset: InternetDataset, exppath: str, renderer=None, rows: Optional[Sequence[int]] = None, result_dir: str = 'result',
                   out_dir: str = 'scene', sink=None) -> List[str]:
    """One picture per video frame with every adapted person of it: for each distinct ``imgname`` among `rows` (default: the rows
    of the dataset's sequences) the frame is decoded once, its people are read from the written ``result/Pred_{n}.pt``
    (``scene_meshes``: order and colours) and drawn over it by one scene pass (``Renderer.render_scenes``, SCENE_BATCH frames per
    call) -> ``scene/<seq>/<frame file stem>.png``.  A pass over written results, not part of the frame step: tracks in lockstep
    reach a video frame at different steps, and ranks own different people.  renderer: a ``render.Renderer`` with the meshes' face
    table (default: the SMPL model's, as the per-person overlays use).  result_dir / out_dir: the folders read and written instead of
    ``result`` and ``scene``.  sink (jpeg.OverlaySink; None: PNG through PIL): the pictures of a scene call go to it in ONE call - with
    --overlay_format jpg the same names with the extension .jpg, with --overlay_video 1 also ``<out_dir>/<seq>.avi``, the frames in
    this order.  -> the written paths, in frame order of first appearance."""
    from PIL import Image
    if rows is None:
        rows = [r for s in dataset.sequences for r in s["rows"]]
    by_frame: Dict[str, List[int]] = {}
    for n in sorted(int(r) for r in rows):
        by_frame.setdefault(str(dataset.imgnames[n]), []).append(n)
    if renderer is None:
        renderer = scene_renderer(None, dataset.device)
    names, paths = list(by_frame), []
    for lo in range(0, len(names), SCENE_BATCH):
        part = names[lo:lo + SCENE_BATCH]
        frames = [torch.from_numpy(dataset.read_frame(name)).to(dataset.device) for name in part]
        scenes = [scene_meshes(dataset, exppath, by_frame[name], int(f.shape[1]), int(f.shape[0]), result_dir=result_dir)
                  for name, f in zip(part, frames)]
        scenes = [[(torch.from_numpy(v).to(dataset.device), torch.from_numpy(c).to(dataset.device), col) for v, c, col in sc] for sc in scenes]
        pics = renderer.render_scenes(frames, scenes)
        targets = [scene_path(exppath, name, out_dir) for name in part]
        for path in targets:
            os.makedirs(os.path.dirname(path), exist_ok=True)
        if sink is not None:
            videos = [os.path.join(exppath, out_dir, (os.path.dirname(name) or "frames") + ".avi") for name in part]
            paths += sink.write(pics, targets, videos)
            continue
        for path, pic in zip(targets, pics):
            Image.fromarray(pic.cpu().numpy()).save(path)
            paths.append(path)
    if sink is not None:
        sink.close()
    return paths


def scene_renderer(assets_bundle, device):
    """The renderer of the scene pass: the face table of the bundle's SMPL model, else of the model files under data/smpl."""
    from .render import Renderer
    if assets_bundle is not None:
        return Renderer(orig_img=True, faces=np.asarray(assets_bundle.smpl_neutral["faces"]), device=device)
    from .smpl import SMPL
    return Renderer(orig_img=True, faces=SMPL("data/smpl", create_transl=False).faces, device=device)


def frame_ids_of(dataset: InternetDataset, sequences):
    """Per sequence the rows' frame numbers, parsed from the trailing digits of the image files' stems - or None unless all parse."""
    import re
    out = []
    for rows in sequences:
        ids = [re.search(r"(\d+)$", os.path.splitext(os.path.basename(str(dataset.imgnames[n])))[0]) for n in rows]
        if any(m is None for m in ids):
            return None
        out.append([int(m.group(1)) for m in ids])
    return out


def smooth_pass(options, dataset: InternetDataset, exppath: str, assets_bundle=None, device=None, rows: Optional[Sequence[int]] = None):
    """--smooth_window H: ``smooth.smooth_results`` over the dataset's sequences (`rows`: only the sequences all of whose rows are
    among them) -> ``result_smooth/Pred_{n}.pt`` with the smoothed frame camera as ``cam_frame`` (``parse_cam`` +
    ``convert_crop_cam_to_orig_img`` on the row's box; the frame's size is read from its file's header, the frame is not decoded) and,
    with --scene_overlays 1 or --compose_only 1, ``scene_smooth/...`` drawn from them."""
    from PIL import Image
    from . import smooth as SM
    from .render import convert_crop_cam_to_orig_img, parse_cam
    from .smpl import SMPL
    if int(getattr(options, "batch_size", 1)) != 1:
        raise ValueError("--smooth_window reads the dumps of a batch-size-1 run (Pred_{n}.pt = row n): pass --batch_size 1")
    done = None if rows is None else {int(r) for r in rows}
    sequences = [list(s["rows"]) for s in dataset.sequences if done is None or all(int(r) in done for r in s["rows"])]
    smpl = (SMPL(tables=assets_bundle.smpl_neutral) if assets_bundle is not None else SMPL("data/smpl", create_transl=False)).to(device)
    sizes: Dict[str, tuple] = {}

    def cam_frame(n, d):
        name = str(dataset.imgnames[n])
        if name not in sizes:
            with Image.open(os.path.join(dataset.img_dir, name)) as im:
                sizes[name] = im.size                                  # (width, height) from the header
        cam = parse_cam(np.asarray(d['cam'], np.float64).reshape(1, 3))
        bbox = np.array([[dataset.centers[n][0], dataset.centers[n][1], float(dataset.scales[n]) * 200]], np.float64)
        return convert_crop_cam_to_orig_img(cam, bbox, sizes[name][0], sizes[name][1])[0].astype(np.float32)

    paths = SM.smooth_results(exppath, sequences, smpl, half_window=int(options.smooth_window), sigma=getattr(options, "smooth_sigma", None),
                              frame_ids=frame_ids_of(dataset, sequences), cam_frame=cam_frame)
    if int(getattr(options, "scene_overlays", 0)) or int(getattr(options, "compose_only", 0)):
        compose_scenes(dataset, exppath, scene_renderer(assets_bundle, device), rows=[n for s in sequences for n in s],
                       result_dir='result_smooth', out_dir='scene_smooth', sink=sink_for(options, dataset.device))
    return paths


def run_driver(options, assets_bundle=None, device=None):
    """``python -m dynaboa_amd.internet``: --extract, or the adaptation of <internet_root> - one stream (the reference), or with
    --split_tracks / --seqs_per_gpu / --num_shards the tracks as sequences."""
    refuse_seq_metrics(options)
    if options.extract:
        if not int(getattr(options, "track", 0)):
            return internet_data_extract(options.extract)
        from .track import rule_of
        return internet_data_extract(options.extract, track=1, device="cuda" if device is None else device, **rule_of(options))
    if int(getattr(options, "track", 0)):
        raise ValueError("--track 1 belongs to --extract DIR: it decides the track array the files are written with")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", options.shard_rank))
    nsh = world if world > 1 else int(options.num_shards)
    if device is None:
        if world > 1:
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        device = torch.device("cuda", torch.cuda.current_device())
    exppath = os.path.join(options.expdir, options.expname)
    scene_pass = int(getattr(options, "scene_overlays", 0)) or int(getattr(options, "compose_only", 0))
    if scene_pass and nsh > 1:
        raise ValueError("--scene_overlays / --compose_only draw the people of ALL ranks into one picture and there are "
                         f"{nsh} shards: run the shards without it, then once more with --compose_only 1 and --num_shards 1")
    smooth = int(getattr(options, "smooth_window", 0))
    if smooth and nsh > 1:
        raise ValueError("--smooth_window smooths whole sequences, written by ALL ranks, and there are "
                         f"{nsh} shards: run the shards without it, then once more with --compose_only 1 and --num_shards 1")
    if getattr(options, "compose_only", 0):
        ds = InternetDataset(options, device=device)
        paths = compose_scenes(ds, exppath, scene_renderer(assets_bundle, device), sink=sink_for(options, device))
        if smooth:
            smooth_pass(options, ds, exppath, assets_bundle, device)
        return paths
    os.makedirs(exppath, exist_ok=True)
    if rank == 0:
        with open(os.path.join(exppath, 'setting.txt'), 'w') as fh:               # dynaboa_internet.py:176-180
            fh.write('------------------ start ------------------\n')
            fh.writelines(f'{k} : {v}\n' for k, v in vars(options).items())
            fh.write('------------------- end -------------------')
    S = int(options.seqs_per_gpu)
    if not (options.split_tracks or S > 1 or nsh > 1):
        ad = Adaptor(options, assets_bundle, device)
        ad.excute()
        if scene_pass:
            compose_scenes(ad.dataset, exppath, scene_renderer(assets_bundle, device), sink=sink_for(options, device))
        if smooth:
            smooth_pass(options, ad.dataset, exppath, assets_bundle, device)
        return list(range(len(ad.dataset)))
    if S > 1:
        from . import native_step as NS
        NS.set_replica_policy(getattr(options, "replica_policy", "throughput") != "bitexact")
    ds = InternetDataset(options, device=device)
    done = run_tracks(options, ds, lambda: Adaptor(copy.copy(options), assets_bundle, device), nsh, rank, S)
    if scene_pass:
        compose_scenes(ds, exppath, scene_renderer(assets_bundle, device), rows=done, sink=sink_for(options, device))
    if smooth:
        smooth_pass(options, ds, exppath, assets_bundle, device, rows=done)
    return done


def main(argv=None):
    return run_driver(parser.parse_args(argv))


if __name__ == '__main__':
    main()
