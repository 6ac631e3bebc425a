#!/usr/bin/env python3
"""Goldens of the 3DPW extraction: the REFERENCE's own ``utils/data_preprocess/pw3d.py::pw3d_extract`` (imported read-only through the
stub recipe of tools/make_golden.py) on a small synthetic sequence file.  Only data is written - the sequence file's arrays and the
arrays of the files the reference writes from them.

What the reference's module needs and this machine lacks is stood in for here:
  * ``cv2``, ``ipdb``, ``tqdm``: empty stubs.  The ``tqdm`` stand-in also yields only the FIRST item of what it wraps: that is how the
    hard-coded list of 24 file names is reduced to one without touching the reference's text.  The synthetic file therefore carries
    the first name of that list.
  * ``numpy.lib.function_base`` (gone from this NumPy) and ``np.bool = bool``.
  * ``model.smpl.SMPL``: the recipe's SMPL stand-in (oracle LBS) on ``assets.make_synthetic_smpl`` tables, seed MALE_SEED for
    gender='male' and FEMALE_SEED for gender='female'.  LBS itself stays unpinned, as everywhere in this project: the goldens pin the
    arithmetic AROUND it, and a test that compares ``j3d`` (or anything computed from it) grants the LBS kernel's own tolerance.
  * ``utils.kp_utils`` is imported as it is.

The sequence (one file, F = 12 frames, two people): a moving camera whose rotation is far from the identity (3DPW's world has y up, the
camera looks along +z with y down), 3DPW-like intrinsics, person 0 male and person 1 female with different ``campose_valid`` masks,
12 betas per person (the reference keeps the first 10).  Asserted here (a seed that misses a condition is replaced, never the
condition): every joint lies in front of the camera at a depth of 2 - 8 m, every mask keeps at least two frames, and every aligned
root angle lies in [0.2, 2.8] rad - away from the ill-conditioned ends of the quaternion route.

  tests/golden/g13_pw3d_sequence.npz   the arrays of the sequence file (tests rebuild the dictionary from them: tests/pw3d_cases.py)
  tests/golden/g13_pw3d_extract.npz    every key of both written files as p<pid>_<key>, plus p<pid>_j3d_model: the stand-in's joints
                                       BEFORE the reference's in-place ``smpl += smpl_trans`` (which writes through a view into the
                                       array it then saves as ``j3d``: the saved ``j3d`` is the fp32 joints PLUS the translation)

usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_pw3d.py [--out tests/golden] [--seed 13]
"""
from __future__ import annotations

import argparse
import os
import pickle
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.dont_write_bytecode = True

import make_golden as MG                        # noqa: E402
from dynaboa_amd import assets                  # noqa: E402
from oracle import ref_cpu as O                 # noqa: E402

F = 12
MALE_SEED, FEMALE_SEED = 1, 2
FIRST_NAME = "downtown_runForBus_00"            # the first entry of the reference's file list (see the module docstring)
VALID = np.array([[1, 1, 0, 1, 1, 1, 1, 0, 1, 1, 1, 1],
                  [0, 1, 1, 1, 1, 0, 0, 1, 1, 1, 0, 1]], dtype=np.uint8)
MODEL_JOINTS = []                               # the stand-in's outputs, copied before the reference can write into them


def rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


def make_sequence(seed):
    rng = np.random.default_rng(seed)
    poses = rng.standard_normal((2, F, 72)) * 0.25
    walk = np.linspace(0.0, 1.0, F)
    for p in range(2):                          # roots tilted about x: with the camera's half turn the aligned angle stays clear of pi
        poses[p, :, :3] = np.stack([(1.3 + 0.3 * p) + 0.3 * walk, 0.4 * walk + 0.1 * rng.standard_normal(F), 0.1 * rng.standard_normal(F)], 1)
    betas = rng.standard_normal((2, 12)) * 0.7
    trans = np.stack([np.stack([-0.6 + 0.9 * walk, 0.9 + 0.02 * np.sin(9 * walk), 0.3 * walk], 1),
                      np.stack([0.7 - 0.4 * walk, 0.85 + 0.02 * np.cos(7 * walk), 0.8 - 0.5 * walk], 1)], 0)
    trans = trans + 0.01 * rng.standard_normal(trans.shape)
    cam_poses = np.tile(np.eye(4), (F, 1, 1))
    for f in range(F):                          # y-up world -> y-down camera (a half turn about x), panning and rolling a little
        R = rot("z", 0.05 * np.sin(5 * walk[f])) @ rot("y", -0.25 + 0.5 * walk[f]) @ rot("x", np.pi - 0.12 + 0.05 * walk[f])
        centre = np.array([0.2 + 0.5 * walk[f], 1.1, 5.4 - 0.8 * walk[f]])       # the camera's position in the world
        cam_poses[f, :3, :3], cam_poses[f, :3, 3] = R, -R @ centre
    K = np.array([[1961.8529, 0.0, 540.0], [0.0, 1969.2309, 960.0], [0.0, 0.0, 1.0]])
    poses2d = np.zeros((2, F, 3, 18))
    poses2d[:, :, 0] = rng.uniform(100.0, 980.0, (2, F, 18))
    poses2d[:, :, 1] = rng.uniform(200.0, 1700.0, (2, F, 18))
    conf = rng.uniform(0.0, 1.0, (2, F, 18))
    conf[conf < 0.15] = 0.0                     # undetected joints: all three entries zero, as OpenPose reports them
    poses2d[:, :, 2] = conf
    poses2d[:, :, :2] *= (conf > 0)[:, :, None, :]
    return dict(poses=poses, betas=betas, trans=trans, poses2d=poses2d, cam_poses=cam_poses, cam_intrinsics=K,
                campose_valid=VALID.copy(), genders=np.array(["m", "f"]), sequence=np.array(FIRST_NAME),
                img_frame_ids=np.arange(F, dtype=np.int64))


def sequence_dict(arrays):
    """The pickled dictionary of a 3DPW sequence file from the arrays of the golden (per-person entries are lists, as in the release).
    tests/pw3d_cases.py holds the same few lines."""
    a = arrays
    n = a["poses"].shape[0]
    return dict(poses=[np.array(a["poses"][p]) for p in range(n)], betas=[np.array(a["betas"][p]) for p in range(n)],
                trans=[np.array(a["trans"][p]) for p in range(n)], poses2d=[np.array(a["poses2d"][p]) for p in range(n)],
                cam_poses=np.array(a["cam_poses"]), cam_intrinsics=np.array(a["cam_intrinsics"]),
                campose_valid=[np.array(a["campose_valid"][p]) for p in range(n)], genders=[str(g) for g in a["genders"]],
                sequence=str(a["sequence"]), img_frame_ids=np.array(a["img_frame_ids"]))


class SMPLStandIn:
    """model.smpl.SMPL of the reference: SMPL(model_dir, gender=..., create_transl=False).to(device)(global_orient=, body_pose=, betas=)."""

    def __init__(self, model_dir=None, gender="neutral", **kw):
        seed = {"male": MALE_SEED, "female": FEMALE_SEED}[gender]
        self.stub = MG.SMPLStub(O.smpl_tables_to_torch(assets.make_synthetic_smpl(seed)))

    def to(self, device):
        return self

    def __call__(self, **kw):
        with torch.no_grad():
            out = self.stub(**kw)
        MODEL_JOINTS.append(out.joints.detach().clone().numpy())
        return out


def load_reference():
    MG.install_stubs()
    for n in ("ipdb", "tqdm"):
        sys.modules[n] = MG._Stub(n)
    sys.modules["tqdm"].tqdm = lambda it, total=None, **kw: (x for i, x in enumerate(it) if i == 0)
    fb = types.ModuleType("numpy.lib.function_base")
    fb.append = np.append
    sys.modules["numpy.lib.function_base"] = fb
    np.bool = bool
    model, smpl = types.ModuleType("model"), types.ModuleType("model.smpl")
    model.__path__ = []
    smpl.SMPL = model.SMPL = SMPLStandIn
    model.smpl = smpl
    sys.modules["model"], sys.modules["model.smpl"] = model, smpl
    os.chdir(MG.REF)
    return MG.load_file("ref_pw3d", "utils/data_preprocess/pw3d.py")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--seed", type=int, default=13)
    a = ap.parse_args()
    out = os.path.abspath(a.out)
    seq = make_sequence(a.seed)
    ref = load_reference()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "sequenceFiles", "test"))
        os.makedirs(os.path.join(tmp, "npz"))
        with open(os.path.join(tmp, "sequenceFiles", "test", FIRST_NAME + ".pkl"), "wb") as fh:
            pickle.dump(sequence_dict(seq), fh, protocol=2)
        ref.pw3d_extract(tmp, os.path.join(tmp, "npz"))
        names = sorted(os.listdir(os.path.join(tmp, "npz")))
        assert names == ["3dpw_0_0.npz", "3dpw_0_1.npz"], names
        files = [dict(np.load(os.path.join(tmp, "npz", n))) for n in names]
    assert len(MODEL_JOINTS) == 2
    payload = {}
    K = seq["cam_intrinsics"]
    for p, d in enumerate(files):
        valid = VALID[p].astype(bool)
        n = int(valid.sum())
        assert n >= 2 and d["j2d"].shape == (n, 49, 3) and d["j3d"].dtype == np.float32, (n, d["j2d"].shape, d["j3d"].dtype)
        # the saved j3d is the model's joints plus the translation, rounded once to fp32 (the in-place += through a view)
        moved = (MODEL_JOINTS[p].astype(np.float64) + seq["trans"][p][valid][:, None, :]).astype(np.float32)
        assert np.array_equal(d["j3d"], moved)
        cam = np.einsum("nij,nkj->nki", seq["cam_poses"][valid][:, :3, :3], d["j3d"].astype(np.float64)) + seq["cam_poses"][valid][:, None, :3, 3]
        assert 2.0 < cam[..., 2].min() and cam[..., 2].max() < 8.0, (cam[..., 2].min(), cam[..., 2].max())
        ang = np.linalg.norm(d["pose"][:, :3], axis=1)
        assert 0.2 <= ang.min() and ang.max() <= 2.8, ang
        assert np.abs(d["j2d"][..., 0] - K[0, 2]).max() < 3000 and np.abs(d["j2d"][..., 1] - K[1, 2]).max() < 3000
        for k, v in d.items():
            payload[f"p{p}_{k}"] = v
        payload[f"p{p}_j3d_model"] = MODEL_JOINTS[p]
        print(f"person {p}: {n} frames, depth {cam[..., 2].min():.2f} .. {cam[..., 2].max():.2f} m, aligned root angle "
              f"{ang.min():.3f} .. {ang.max():.3f} rad, dtypes", {k: str(v.dtype) for k, v in d.items()})
    os.makedirs(out, exist_ok=True)
    np.savez_compressed(os.path.join(out, "g13_pw3d_sequence.npz"), **seq)
    np.savez_compressed(os.path.join(out, "g13_pw3d_extract.npz"), **payload)
    print("g13 ok")


if __name__ == "__main__":
    main()
