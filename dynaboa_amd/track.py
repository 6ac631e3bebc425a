"""Person ids for detections that come without them (csrc/track.hip; the rule is stated at dyb_track_videos in include/dynaboa_hip.h).

Every multi-person path of this project starts from a person id: ``internet.py`` reads AlphaPose's ``idx`` into the ``track`` array,
and ``--split_tracks 1``, the lockstep groups, the scene overlays, per-track videos and smoothing hang on it.  AlphaPose writes
``idx`` only when it ran with pose tracking, and OpenPose - the reference's own live detector - never gives ids.  The reference leaves
association to external tools; this module is the missing link between raw detections and everything downstream of an id:

  track_videos       a batch of videos -> ids: ONE packed upload, ONE ``dyb_track_videos`` call (a workgroup per video), one download;
  the command line   ``python -m dynaboa_amd.track --openpose DIR [--frames DIR] --out DIR [--min_track_frames N] [rule flags]``: every
                     ``<stem>_keypoints.json`` of DIR, ALL ``people`` of each -> ``track<id>.npz`` per kept track (``imgname``,
                     ``keypoints (N, 25, 3)``: what ``python -m dynaboa_amd.online --detections FILE`` reads) and ``tracks.json``.

The rule is greedy keypoint similarity against each track's last detection.  Its limits: 64 live people per video, 32 joints, no
motion model (no constant-velocity prediction), no appearance term and no re-identification - a person lost for more than ``max_age``
frame ids comes back under a new id."""
from __future__ import annotations

import argparse
import glob
import json
import os
import re
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

MAX_PEOPLE, MAX_KP, VIDEO_INTS = 64, 32, 4     # DYB_TRACK_MAX_PEOPLE, DYB_TRACK_MAX_KP, DYB_TRACK_VIDEO_INTS
C_MIN = 0.3                                    # internet.CONF_THRESHOLD: the confidence above which the project counts a joint
KAPPA, S_MIN, MAX_AGE, MIN_COMMON = 0.1, 0.3, 5, 3
COUNT_NAMES = ("started", "untrackable", "no_slot")


def track_videos(videos, frame_ids=None, *, c_min: float = C_MIN, kappa: float = KAPPA, s_min: float = S_MIN, max_age: int = MAX_AGE,
                 min_common: int = MIN_COMMON, strict: bool = False, device="cuda"):
    """videos: a list of videos, each a list of per-frame (n_f, K, 3) arrays of (x, y, confidence) in pixels - empty frames and empty
    videos are allowed, K is one value for the whole call.  frame_ids: per video the frames' numbers, strictly increasing (None:
    their positions).  -> (tracks, sims, counts): tracks and sims in the nesting of `videos` - per frame an (n_f,) int32 array of ids
    (-1: none) and an (n_f,) float32 array of the similarity a detection was matched with (0: it started a track, -1: none) - and
    counts, per video a dict(started=, untrackable=, no_slot=).  ValueError: frames of different K, frame ids that do not increase
    and, with strict=True, a frame of more than 64 detections (strict=False: the rule applies - the 65th onward get -1)."""
    from . import _lib
    from ._abi import check
    from .hmr import stream_of
    frames = [np.asarray(f, np.float32) for v in videos for f in v]
    shapes = {f.shape[1:] for f in frames if f.ndim == 3}
    if any(f.ndim != 3 for f in frames if f.size) or len(shapes) > 1 or any(s[1] != 3 for s in shapes):
        raise ValueError(f"track_videos: every frame must be (n, K, 3) with one K, got {sorted(shapes)}")
    K = shapes.pop()[0] if shapes else 1
    if not 1 <= K <= MAX_KP:
        raise ValueError(f"track_videos: K = {K} outside 1..{MAX_KP}")
    frames = [f.reshape(-1, K, 3) for f in frames]
    if strict and any(f.shape[0] > MAX_PEOPLE for f in frames):
        raise ValueError(f"track_videos: a frame with {max(f.shape[0] for f in frames)} detections (at most {MAX_PEOPLE} are tracked)")
    lengths = [len(v) for v in videos]
    fid = None
    if frame_ids is not None:
        if [len(x) for x in frame_ids] != lengths:
            raise ValueError("track_videos: frame_ids must list one id per frame of every video")
        for x in frame_ids:
            if any(int(b) <= int(a) for a, b in zip(x[:-1], x[1:])):
                raise ValueError("track_videos: frame ids must increase strictly within a video")
        fid = np.array([int(i) for x in frame_ids for i in x], np.int32)
    V, F = len(videos), len(frames)
    if V == 0:
        return [], [], []
    counts_f = [f.shape[0] for f in frames]
    n = int(sum(counts_f))
    det_off = np.concatenate([[0], np.cumsum(counts_f)]).astype(np.int32)
    frame_off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    # one upload: the keypoints' bits and the three integer tables in one int32 buffer
    words = [np.concatenate(frames).reshape(-1).view(np.int32) if n else np.zeros(0, np.int32), det_off, frame_off,
             fid if fid is not None else np.zeros(0, np.int32)]
    starts = np.concatenate([[0], np.cumsum([w.size for w in words])])
    dev = torch.device(device)
    buf = torch.from_numpy(np.concatenate(words)).to(dev)
    part = lambda i: buf[int(starts[i]):int(starts[i + 1])]
    out = torch.empty(2 * n + VIDEO_INTS * V, dtype=torch.int32, device=dev)      # track | sim bits | video
    ptr = lambda t: t.data_ptr() if t.numel() else None
    check(_lib.load().dyb_track_videos(ptr(part(0)), part(1).data_ptr(), part(2).data_ptr(), ptr(part(3)) if fid is not None else None, K,
                                       float(c_min), float(kappa), float(s_min), int(max_age), int(min_common), ptr(out[:n]),
                                       ptr(out[n:2 * n]), out[2 * n:].data_ptr(), n, F, V, stream_of(buf)), "dyb_track_videos")
    host = out.cpu().numpy()
    track, sim, video = host[:n], host[n:2 * n].view(np.float32), host[2 * n:].reshape(V, VIDEO_INTS)
    tracks, sims, f = [], [], 0
    for L in lengths:
        tracks.append([track[det_off[i]:det_off[i + 1]].copy() for i in range(f, f + L)])
        sims.append([sim[det_off[i]:det_off[i + 1]].copy() for i in range(f, f + L)])
        f += L
    return tracks, sims, [dict(zip(COUNT_NAMES, (int(c) for c in row[:3]))) for row in video]


def trailing_ids(stems: Sequence[str]) -> Optional[List[int]]:
    """The numbers in the trailing digits of `stems` - or None unless every stem has them and they increase strictly."""
    found = [re.search(r"(\d+)$", s) for s in stems]
    if any(m is None for m in found):
        return None
    ids = [int(m.group(1)) for m in found]
    return ids if all(b > a for a, b in zip(ids[:-1], ids[1:])) else None


def read_openpose(folder: str, frame_names: Optional[Sequence[str]] = None):
    """Every ``<stem>_keypoints.json`` of `folder` in name order, ALL people of each -> (names, people, frame_ids): names[i] the frame
    file of `frame_names` with that stem (the stem where there is none), people[i] an (n_i, 25, 3) float32 array, frame_ids from the
    stems' trailing digits when every stem parses and they increase (else None: positions)."""
    stems_of = {os.path.splitext(n)[0]: n for n in (frame_names or [])}
    stems, people = [], []
    for f in sorted(glob.glob(os.path.join(folder, "*_keypoints.json"))):
        with open(f) as fh:
            rec = json.load(fh).get("people", [])
        stems.append(os.path.basename(f)[:-len("_keypoints.json")])
        people.append(np.asarray([p["pose_keypoints_2d"] for p in rec], dtype=np.float32).reshape(-1, 25, 3))
    return [stems_of.get(s, s) for s in stems], people, trailing_ids(stems)


def split_tracks(names: Sequence[str], people: Sequence[np.ndarray], tracks: Sequence[np.ndarray], min_track_frames: int = 1) -> Dict[int, dict]:
    """-> {id: dict(imgname=[...], keypoints=(N, K, 3), positions=[...])} for the tracks with at least `min_track_frames` frames, in id
    order; positions are the frames' indices in `names`."""
    out: Dict[int, dict] = {}
    for i, (kp, tr) in enumerate(zip(people, tracks)):
        for d, t in enumerate(tr):
            if t >= 0:
                e = out.setdefault(int(t), dict(imgname=[], keypoints=[], positions=[]))
                e["imgname"].append(names[i]); e["keypoints"].append(kp[d]); e["positions"].append(i)
    return {t: dict(imgname=e["imgname"], keypoints=np.stack(e["keypoints"]).astype(np.float32), positions=e["positions"])
            for t, e in sorted(out.items()) if len(e["imgname"]) >= int(min_track_frames)}


def rule_of(options) -> dict:
    return dict(c_min=options.c_min, kappa=options.kappa, s_min=options.s_min, max_age=options.max_age, min_common=options.min_common)


def track_openpose(folder: str, out: str, frame_names: Optional[Sequence[str]] = None, min_track_frames: int = 1, device="cuda", **rule):
    """The command line's work: read `folder`, one ``track_videos`` call, ``<out>/track<id>.npz`` per kept track and
    ``<out>/tracks.json`` (per track: id, first and last frame, frames; then the counts).  -> {id: path of its npz}."""
    names, people, ids = read_openpose(folder, frame_names)
    tracks, _, counts = track_videos([people], None if ids is None else [ids], device=device, **rule)
    kept = split_tracks(names, people, tracks[0], min_track_frames)
    os.makedirs(out, exist_ok=True)
    paths, rows = {}, []
    for t, e in kept.items():
        paths[t] = os.path.join(out, f"track{t}.npz")
        np.savez(paths[t], imgname=np.array(e["imgname"]), keypoints=e["keypoints"])
        rows.append(dict(id=t, first=e["imgname"][0], last=e["imgname"][-1], frames=len(e["imgname"])))
    with open(os.path.join(out, "tracks.json"), "w") as fh:
        json.dump(dict(tracks=rows, counts=counts[0], frames=len(names), min_track_frames=int(min_track_frames)), fh, indent=1)
    return paths


def add_rule_arguments(p):
    p.add_argument('--c_min', type=float, default=C_MIN, help='a joint is visible iff its confidence is above this')
    p.add_argument('--kappa', type=float, default=KAPPA, help='width of the per-joint similarity, relative to the square root of the body area')
    p.add_argument('--s_min', type=float, default=S_MIN, help='similarity below which a detection does not continue a track, in (0, 1]')
    p.add_argument('--max_age', type=int, default=MAX_AGE, help='frame ids a track survives without a detection')
    p.add_argument('--min_common', type=int, default=MIN_COMMON, help='visible joints a detection needs, and joints a pair must share')


def _make_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--openpose', type=str, required=True, metavar='DIR', help='directory of OpenPose <stem>_keypoints.json files')
    p.add_argument('--frames', type=str, default=None, metavar='DIR', help="directory of the frames: imgname holds their file names")
    p.add_argument('--out', type=str, required=True, metavar='DIR')
    p.add_argument('--min_track_frames', type=int, default=1, help='drop tracks with fewer frames')
    add_rule_arguments(p)
    return p


def frame_files(folder: Optional[str]) -> Optional[List[str]]:
    if not folder:
        return None
    return sorted(n for n in os.listdir(folder) if n.lower().endswith((".png", ".jpg", ".jpeg", ".bmp")))


def main(argv=None, device="cuda"):
    o = _make_parser().parse_args(argv)
    paths = track_openpose(o.openpose, o.out, frame_files(o.frames), o.min_track_frames, device=device, **rule_of(o))
    print(f"{len(paths)} tracks -> {o.out}")
    return paths


if __name__ == '__main__':
    main()
