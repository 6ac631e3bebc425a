"""3DPW sequence files -> the loader's ``3dpw_<seq>_<pid>.npz`` files (reference ``utils/data_preprocess/pw3d.py::pw3d_extract``),
on the device: per person the gendered SMPL forward of this project (csrc/smpl_lbs.hip) in chunks of frames, each followed by one
launch of ``dyb_pw3d_annotate`` (csrc/pw3d_extract.hip: projection of the 49 joints, box, root alignment).  ``datasets.PW3D``
reads the written files as they are.

    python -m dynaboa_amd.pw3d_extract --pw3d_root DIR --out DIR [--split S] [--order FILE] [--smpl_dir DIR] [--check DIR]

Written keys and dtypes are the reference's: ``imgname`` (str), ``gender`` (one 'm' / 'f' per frame), ``scale`` / ``center`` / ``j2d``
/ ``op_j2d`` (fp64), ``pose`` / ``shape`` (the sequence file's dtype; ``pose[:, :3]`` holds the aligned root, an fp32 value),
``j3d`` (fp32).  ``j3d`` is what the reference SAVES, not what its name suggests: its ``projection`` adds the translation in place
through a view of the array it later saves, so the file holds ``(float)((double)joint + trans)`` - the very points that are
projected.  This module writes the same.

Rules of this project's own, where the reference has none or breaks:
  * a person with ONE valid frame is handled like any other (the reference's ``.squeeze()`` drops the batch axis and fails);
  * a person with NO valid frame writes no file, and the other people keep their ``p_id``;
  * a gender other than 'm' or 'f' raises ``ValueError`` before anything of that sequence is written;
  * the caller's sequence dictionary is never written;
  * the order of the files is an argument (``order``); for ``split='test'`` it defaults to the order of the reference's released
    files (``constants.PW3D_TEST_ORDER``), for other splits to the sorted directory listing.  A name that is not on disk is an error.
"""
from __future__ import annotations

import argparse
import os
import pickle
import sys
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, constants as C
from ._abi import check
from .hmr import stream_of
from .smpl import SMPL

# --check: largest deviation a numeric key may show against the compared file.  The two sides differ only by the fp32 LBS of two
# implementations (a few ulp at |p| ~ 5 m: some 1e-6 m, times focal / depth ~ 1000 px / m: some 1e-3 px); the bounds leave a
# factor of ~25 over that and are far below anything an annotation means.  `pose` is compared as [:, :3] (aligned root, bound
# below) and [:, 3:] (copied: equal); every other key must be equal.
CHECK_TOL = dict(j3d=1e-4, j2d=0.05, center=0.05, scale=0.05 / 200.0, pose_root=1e-4)


def annotate(joints49: torch.Tensor, trans: torch.Tensor, cam_pose: torch.Tensor, cam_intrinsics: torch.Tensor,
             root_aa: torch.Tensor) -> Dict[str, torch.Tensor]:
    """``dyb_pw3d_annotate`` on device tensors: joints49 fp32 (n, 49, 3) before translation, trans fp64 (n, 3), cam_pose fp64
    (n, 4, 4), cam_intrinsics fp64 (3, 3), root_aa fp32 (n, 3) -> {'j2d' fp64 (n, 49, 3), 'center' fp64 (n, 2), 'scale' fp64 (n,),
    'root_aligned' fp32 (n, 3)}."""
    n = joints49.shape[0]
    want = ((joints49, torch.float32, (n, 49, 3)), (trans, torch.float64, (n, 3)), (cam_pose, torch.float64, (n, 4, 4)),
            (cam_intrinsics, torch.float64, (3, 3)), (root_aa, torch.float32, (n, 3)))
    for t, dt, shape in want:
        if t.dtype != dt or tuple(t.shape) != shape or t.device != joints49.device:
            raise ValueError(f"annotate: expected {dt} {shape} on {joints49.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    if n == 0:
        raise ValueError("annotate: no frames")
    j, t, p, k, r = (x.contiguous() for x in (joints49, trans, cam_pose, cam_intrinsics, root_aa))
    dev = j.device
    out = dict(j2d=torch.empty(n, 49, 3, dtype=torch.float64, device=dev), center=torch.empty(n, 2, dtype=torch.float64, device=dev),
               scale=torch.empty(n, dtype=torch.float64, device=dev), root_aligned=torch.empty(n, 3, dtype=torch.float32, device=dev))
    check(_lib.load().dyb_pw3d_annotate(j.data_ptr(), t.data_ptr(), p.data_ptr(), k.data_ptr(), r.data_ptr(), out["j2d"].data_ptr(),
                                        out["center"].data_ptr(), out["scale"].data_ptr(), out["root_aligned"].data_ptr(), n,
                                        stream_of(j)), "dyb_pw3d_annotate")
    return out


def extract_sequence(data: dict, seq_idx: int, out_dir: str, smpl_male, smpl_female, device, chunk: int = 1024) -> List[str]:
    """One loaded sequence dictionary -> ``3dpw_{seq_idx}_{p_id}.npz`` per person with a valid frame; returns the written paths."""
    device = torch.device(device)
    num_people, num_frames = len(data['poses']), len(data['img_frame_ids'])
    genders = [str(g) for g in data['genders']]
    for g in genders[:num_people]:
        if g not in ('m', 'f'):
            raise ValueError(f"3DPW gender must be 'm' or 'f', got {g!r} (sequence {data['sequence']})")
    seq_name = str(data['sequence'])
    names = np.array(['imageFiles/' + seq_name + '/image_%05d.jpg' % i for i in range(num_frames)])
    cam_poses = np.asarray(data['cam_poses'], dtype=np.float64)
    K = torch.from_numpy(np.ascontiguousarray(data['cam_intrinsics'], dtype=np.float64)).to(device)
    slots = list(C.PW3D_OP18_SLOTS)
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for p_id in range(num_people):
        valid = np.asarray(data['campose_valid'][p_id]).astype(bool)
        n = int(valid.sum())
        if n == 0:
            continue
        poses = np.array(data['poses'][p_id])[valid]                       # (boolean indexing copies: the caller's arrays stay)
        shapes = np.tile(np.asarray(data['betas'][p_id])[:10].reshape(1, -1), (num_frames, 1))[valid]
        op = np.asarray(data['poses2d'][p_id]).transpose(0, 2, 1)[valid]
        op_j2d = np.zeros((n, 49, 3), dtype=np.float64)
        op_j2d[:, slots] = op
        smpl = smpl_male if genders[p_id] == 'm' else smpl_female

        pose_t = torch.from_numpy(poses.astype(np.float32)).to(device)
        betas_t = torch.from_numpy(shapes.astype(np.float32)).to(device)
        trans_t = torch.from_numpy(np.asarray(data['trans'][p_id], dtype=np.float64)[valid]).to(device)
        cam_t = torch.from_numpy(cam_poses[valid]).to(device)
        parts: Dict[str, list] = dict(j3d=[], j2d=[], center=[], scale=[], root_aligned=[])
        with torch.no_grad():
            for lo in range(0, n, chunk):
                hi = min(n, lo + chunk)
                joints = smpl(betas=betas_t[lo:hi], body_pose=pose_t[lo:hi, 3:], global_orient=pose_t[lo:hi, :3]).joints
                a = annotate(joints, trans_t[lo:hi], cam_t[lo:hi], K, pose_t[lo:hi, :3])
                parts["j3d"].append((joints.double() + trans_t[lo:hi, None, :]).float())     # see the module docstring
                for k in ("j2d", "center", "scale", "root_aligned"):
                    parts[k].append(a[k])
        host = {k: torch.cat(v, 0).cpu().numpy() for k, v in parts.items()}
        poses[:, :3] = host["root_aligned"]
        path = os.path.join(out_dir, f'3dpw_{seq_idx}_{p_id}.npz')
        np.savez(path, imgname=names[valid], gender=np.array([genders[p_id]] * n), scale=host["scale"], center=host["center"],
                 pose=poses, shape=shapes, j3d=host["j3d"], j2d=host["j2d"], op_j2d=op_j2d)
        written.append(path)
    return written


def sequence_order(seq_dir: str, split: str = 'test', order: Optional[Sequence[str]] = None) -> List[str]:
    """The file names of ``seq_dir`` in extraction order; a name of ``order`` that is not on disk is an error that names it."""
    if order is None:
        order = [n + '.pkl' for n in C.PW3D_TEST_ORDER] if split == 'test' else sorted(f for f in os.listdir(seq_dir) if f.endswith('.pkl'))
    order = list(order)
    for name in order:
        if not os.path.isfile(os.path.join(seq_dir, name)):
            raise FileNotFoundError(f"3DPW sequence file {name!r} is not in {seq_dir}")
    return order


def pw3d_extract(dataset_path: str, out_path: str, split: str = 'test', order: Optional[Sequence[str]] = None, smpl_male=None,
                 smpl_female=None, smpl_dir: str = "data/smpl", device="cuda", chunk: int = 1024) -> List[str]:
    """Every sequence file of ``dataset_path/sequenceFiles/<split>/`` in ``order`` (see ``sequence_order``); the position in the
    order is the file's ``seq_idx``.  Returns the written paths."""
    seq_dir = os.path.join(dataset_path, 'sequenceFiles', split)
    order = sequence_order(seq_dir, split, order)
    if smpl_male is None:
        smpl_male = SMPL(smpl_dir, gender='male', create_transl=False).to(device)
    if smpl_female is None:
        smpl_female = SMPL(smpl_dir, gender='female', create_transl=False).to(device)
    written = []
    for seq_idx, name in enumerate(order):
        with open(os.path.join(seq_dir, name), 'rb') as fh:
            data = pickle.load(fh, encoding='latin1')
        written += extract_sequence(data, seq_idx, out_path, smpl_male, smpl_female, device, chunk)
    return written


def check_files(written: Sequence[str], check_dir: str):
    """Compare every written file with the same-named file of ``check_dir``.  -> (ok, {key: largest deviation}, [problems]).
    A missing file or key, a shape, an ``imgname``, a ``gender`` or any other exact key that differs, or a numeric key beyond
    CHECK_TOL is a problem."""
    worst: Dict[str, float] = {}
    problems: List[str] = []
    for path in written:
        name = os.path.basename(path)
        other = os.path.join(check_dir, name)
        if not os.path.isfile(other):
            problems.append(f"{name}: not in {check_dir}")
            continue
        a, b = np.load(path), np.load(other)
        if sorted(a.files) != sorted(b.files):
            problems.append(f"{name}: keys {sorted(a.files)} != {sorted(b.files)}")
            continue
        for k in a.files:
            x, y = a[k], b[k]
            if x.shape != y.shape:
                problems.append(f"{name}: {k} has shape {x.shape}, expected {y.shape}")
                continue
            if x.dtype.kind in "US":
                if not np.array_equal(x, y):
                    problems.append(f"{name}: {k} differs")
                continue
            pieces = (("pose_root", x[:, :3], y[:, :3]), ("pose_body", x[:, 3:], y[:, 3:])) if k == "pose" else ((k, x, y),)
            for label, u, v in pieces:
                dev = float(np.abs(u.astype(np.float64) - v.astype(np.float64)).max()) if u.size else 0.0
                if not np.isfinite(dev):
                    dev = 0.0 if np.array_equal(u, v, equal_nan=True) else float("inf")
                worst[label] = max(worst.get(label, 0.0), dev)
                if dev > CHECK_TOL.get(label, 0.0):
                    problems.append(f"{name}: {label} deviates by {dev:.3e} (allowed {CHECK_TOL.get(label, 0.0):.1e})")
    return not problems, worst, problems


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m dynaboa_amd.pw3d_extract", description=__doc__.split("\n\n")[0])
    ap.add_argument("--pw3d_root", required=True, help="the 3DPW release (holds sequenceFiles/<split>/*.pkl)")
    ap.add_argument("--out", required=True, help="directory the 3dpw_<seq>_<pid>.npz files are written to")
    ap.add_argument("--split", default="test")
    ap.add_argument("--order", default=None, help="text file, one sequence file name per line (default: see the module docstring)")
    ap.add_argument("--smpl_dir", default="data/smpl", help="directory of SMPL_MALE.pkl / SMPL_FEMALE.pkl")
    ap.add_argument("--check", default=None, help="directory of reference npz files to compare the written files with")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--chunk", type=int, default=1024)
    a = ap.parse_args(argv)
    order = None
    if a.order is not None:
        with open(a.order) as fh:
            order = [ln.strip() for ln in fh if ln.strip()]
    written = pw3d_extract(a.pw3d_root, a.out, split=a.split, order=order, smpl_dir=a.smpl_dir, device=a.device, chunk=a.chunk)
    print(f"wrote {len(written)} files to {a.out}")
    if a.check is None:
        return 0
    ok, worst, problems = check_files(written, a.check)
    for k in sorted(worst):
        print(f"check {k}: largest deviation {worst[k]:.3e}")
    for p in problems:
        print("check FAILED:", p)
    print("check", "ok" if ok else "failed")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
