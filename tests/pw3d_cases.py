"""Cases of the 3DPW extraction, shared by tests/test_pw3d_extract_emu.py (host build of the product sources, torch on the CPU) and
tests/test_pw3d_extract_gpu.py (MI355X).

Kernel cases (``case_*`` taking a backend of tests/backends.py) drive ``dyb_pw3d_annotate`` through the C ABI against the fp64 NumPy
restatement below and against golden g13 (tools/make_golden_pw3d.py: the reference's own pw3d_extract on a synthetic sequence).
Module cases (taking a torch device) drive ``dynaboa_amd.pw3d_extract``; on the emulator the library is swapped in with
``_lib.use_library``, so SMPL and ``annotate`` run the same host-compiled kernels on CPU tensors - nothing is injected or faked
except, for the command, the reader of SMPL_*.pkl files (the test hands over synthetic tables instead).

Bounds:
  * j2d / center / scale against the restatement: the two sides do the same fp64 operations and differ only in the order of the
    4-term and 3-term sums and in fused multiply-adds: ``pixel_bound`` = 32 * 2^-53 * max|coordinate| of the case (about 1e-11 px).
  * root_aligned: what the existing rotation-matrix-to-axis-angle kernel test grants against golden g1, R2AA_RTOL / R2AA_ATOL
    (tests/kernel_cases.py:626, ``assert_allclose(aa, g["r2aa_out"], rtol=1e-4, atol=2e-6)``).
  * module level, where the joints come from the LBS kernel and the golden's from the oracle's LBS (LBS is unpinned everywhere in
    this project): j3d within LBS_TOL = kernel_cases.TOL (the bound of case_lbs, tests/kernel_cases.py:677) times the largest model
    joint, plus one fp32 rounding of the translated point; j2d / center / scale within that times f / z_min plus the kernel bound.
"""
from __future__ import annotations

import os
import pickle

import numpy as np
import torch

from conftest import golden
from kernel_cases import TOL as LBS_TOL

NJ = 49
NS = (1, 3, 4, 5, 67)                     # below, at and across the 4 frames of a workgroup (PW_WAVES, csrc/pw3d_extract.hip), many workgroups
R2AA_RTOL, R2AA_ATOL = 1e-4, 2e-6         # tests/kernel_cases.py:626
MALE_SEED, FEMALE_SEED = 1, 2             # tools/make_golden_pw3d.py


def pixel_bound(*arrays):
    return 32.0 * 2.0 ** -53 * max(float(np.abs(a).max()) for a in arrays)


# ---------------------------------------------------------------------------------------- the restatement
def restate(joints49, trans, cam_pose, K, round32=True):
    """fp64 NumPy: projection, box.  round32=False leaves out the one fp32 rounding of joint + trans."""
    p = joints49.astype(np.float64) + trans[:, None, :]
    if round32:
        p = p.astype(np.float32).astype(np.float64)
    ph = np.concatenate([p, np.ones(p.shape[:2] + (1,))], -1)
    q = np.einsum("nrk,njk->njr", cam_pose[:, :3, :], ph)
    q = q / q[..., 2:3]
    uv = np.einsum("rk,njk->njr", K, q)[..., :2]
    j2d = np.concatenate([uv, np.ones(uv.shape[:2] + (1,))], -1)
    lo, hi = uv.min(1), uv.max(1)
    return dict(j2d=j2d, center=(hi + lo) / 2.0, scale=(hi - lo).max(1) / 200.0)


def rodrigues64(aa):
    """Rotation matrix of an axis-angle vector, fp64 (the plain formula: every route to a rotation matrix agrees to rounding)."""
    th = np.linalg.norm(aa, axis=-1)[..., None, None]
    k = aa / np.maximum(np.linalg.norm(aa, axis=-1, keepdims=True), 1e-300)
    Kx = np.zeros(aa.shape[:-1] + (3, 3))
    Kx[..., 0, 1], Kx[..., 0, 2], Kx[..., 1, 0] = -k[..., 2], k[..., 1], k[..., 2]
    Kx[..., 1, 2], Kx[..., 2, 0], Kx[..., 2, 1] = -k[..., 0], -k[..., 1], k[..., 0]
    return np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)


def log64(R):
    """Axis-angle of a rotation matrix, fp64, by trace and antisymmetric part (well conditioned for angles in [0.2, 2.8])."""
    c = np.clip((np.trace(R, axis1=-2, axis2=-1) - 1.0) / 2.0, -1.0, 1.0)
    th = np.arccos(c)
    w = np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    return w * (th / (2.0 * np.sin(th)))[..., None]


def restate_root(root_aa, cam_pose):
    Rc = cam_pose[:, :3, :3].astype(np.float32).astype(np.float64)
    return log64(Rc @ rodrigues64(root_aa.astype(np.float64)))


# ---------------------------------------------------------------------------------------- seeded inputs in 3DPW's ranges
def make_inputs(n, seed, trans_about=2.0):
    """Depths 2 - 8 m, focal about 1960 px, principal point about (540, 960), a camera turned half round about x (3DPW's world has y
    up), |trans| about `trans_about`; the aligned root angle lies in [0.3, 2.7] rad by construction."""
    rng = np.random.default_rng(seed)
    joints = (rng.standard_normal((n, NJ, 3)) * 0.35).clip(-0.95, 0.95).astype(np.float32)
    d = rng.standard_normal((n, 3))
    trans = trans_about * d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.9, 1.1, (n, 1))
    Rc = rodrigues64(np.array([np.pi, 0.0, 0.0]) + 0.3 * rng.standard_normal((n, 3)))
    in_cam = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(3.0, 7.0, n)], 1)     # where the person stands
    cam_pose = np.tile(np.eye(4), (n, 1, 1))
    cam_pose[:, :3, :3] = Rc
    cam_pose[:, :3, 3] = in_cam - np.einsum("nij,nj->ni", Rc, trans)
    K = np.array([[1961.0 + rng.uniform(-5, 5), 0.0, 540.0 + rng.uniform(-3, 3)], [0.0, 1969.0 + rng.uniform(-5, 5), 960.0 + rng.uniform(-3, 3)],
                  [0.0, 0.0, 1.0]])
    ax = rng.standard_normal((n, 3))
    want = ax / np.linalg.norm(ax, axis=1, keepdims=True) * rng.uniform(0.3, 2.7, (n, 1))                  # the aligned rotation
    root = log64(np.swapaxes(Rc, 1, 2) @ rodrigues64(want)).astype(np.float32)
    return joints, trans, cam_pose, K, root


def run_annotate(be, joints, trans, cam_pose, K, root):
    n = joints.shape[0]
    f64 = lambda shape: be.dev(np.full(shape, np.nan), np.float64)
    j2d, center, scale, ra = f64((n, NJ, 3)), f64((n, 2)), f64((n,)), be.empty((n, 3))
    rc = be.lib.dyb_pw3d_annotate(be.ptr(be.dev(joints)), be.ptr(be.dev(trans, np.float64)), be.ptr(be.dev(cam_pose, np.float64)),
                                  be.ptr(be.dev(K, np.float64)), be.ptr(be.dev(root)), be.ptr(j2d), be.ptr(center), be.ptr(scale),
                                  be.ptr(ra), n, be.stream)
    assert rc == 0, rc
    return dict(j2d=be.host(j2d), center=be.host(center), scale=be.host(scale), root_aligned=be.host(ra))


def compare(out, ref, bound, what=""):
    for k in ("j2d", "center", "scale"):
        err = float(np.abs(out[k] - ref[k]).max())
        print(f"{what} {k}: max deviation {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (what, k, err, bound)


def case_seeded(be, n):
    joints, trans, cam_pose, K, root = make_inputs(n, seed=100 + n)
    out = run_annotate(be, joints, trans, cam_pose, K, root)
    ref = restate(joints, trans, cam_pose, K)
    compare(out, ref, pixel_bound(ref["j2d"]), f"n={n}")
    assert np.array_equal(out["j2d"][..., 2], np.ones((n, NJ)))
    np.testing.assert_allclose(out["root_aligned"], restate_root(root, cam_pose), rtol=R2AA_RTOL, atol=R2AA_ATOL)


def case_rounding(be, n=5):
    """Translations near 5 m: the fp32 rounding of joint + trans (half an ulp of 2.4e-7 m at 4 - 8 m, times focal / depth) moves a pixel
    coordinate by far more than the fp64 bound.  The kernel matches the restatement WITH the rounding and not the one without."""
    joints, trans, cam_pose, K, root = make_inputs(n, seed=7, trans_about=5.0)
    out = run_annotate(be, joints, trans, cam_pose, K, root)
    ref, plain = restate(joints, trans, cam_pose, K), restate(joints, trans, cam_pose, K, round32=False)
    bound = pixel_bound(ref["j2d"])
    compare(out, ref, bound, "rounded")
    gap = float(np.abs(out["j2d"] - plain["j2d"]).max())
    print(f"unrounded restatement differs by {gap:.3e} px (bound {bound:.3e})")
    assert gap > 1000.0 * bound, (gap, bound)
    assert float(np.abs(out["center"] - plain["center"]).max()) > bound


def case_lanes(be, sign):
    """The extrema come from joints 0, 47 and 48 (first lane, last two lanes that hold a joint), and every coordinate lies on one side
    of the origin (sign = +1: all positive, -1: all negative through a negative principal point), so a contribution of the idle
    lanes 49..63 - a zero, say - would show as a minimum (or maximum) of 0.  Two frames with the roles of the joints swapped."""
    rng = np.random.default_rng(3)
    n = 2
    joints = np.zeros((n, NJ, 3), np.float32)
    joints[..., :2] = rng.uniform(-0.3, 0.3, (n, NJ, 2))
    joints[0, 0, :2], joints[0, 47, 0], joints[0, 48, 1] = (0.9, 0.9), -0.9, -0.9          # maxima in lane 0, minima in lanes 47 / 48
    joints[1, 0, :2], joints[1, 47, 0], joints[1, 48, 1] = (-0.9, -0.9), 0.9, 0.9
    trans = np.tile(np.array([0.0, 0.0, 4.0]), (n, 1))
    cam_pose = np.tile(np.eye(4), (n, 1, 1))
    K = np.array([[1961.0, 0.0, sign * 3000.0], [0.0, 1969.0, sign * 3000.0], [0.0, 0.0, 1.0]])
    root = np.tile(np.array([0.4, -0.7, 0.3], np.float32), (n, 1))
    out = run_annotate(be, joints, trans, cam_pose, K, root)
    ref = restate(joints, trans, cam_pose, K)
    assert (sign * ref["j2d"][..., :2] > 0).all()
    compare(out, ref, pixel_bound(ref["j2d"]), f"lanes sign={sign}")
    u, v = out["j2d"][..., 0], out["j2d"][..., 1]
    for f in range(n):
        assert out["center"][f, 0] == (max(u[f, 0], u[f, 47]) + min(u[f, 0], u[f, 47])) / 2.0
        assert out["center"][f, 1] == (max(v[f, 0], v[f, 48]) + min(v[f, 0], v[f, 48])) / 2.0


def person_rows(seq, ext, p):
    valid = seq["campose_valid"][p].astype(bool)
    return valid, dict(joints=ext[f"p{p}_j3d_model"], trans=seq["trans"][p][valid], cam_pose=seq["cam_poses"][valid],
                       K=seq["cam_intrinsics"], root=seq["poses"][p][valid][:, :3].astype(np.float32))


def case_golden_kernel(be):
    """The kernel on the joints the reference itself projected (golden g13: the stand-in's joints before the translation)."""
    seq, ext = golden("g13_pw3d_sequence.npz"), golden("g13_pw3d_extract.npz")
    for p in range(2):
        _, r = person_rows(seq, ext, p)
        out = run_annotate(be, r["joints"], r["trans"], r["cam_pose"], r["K"], r["root"])
        ref = {k: ext[f"p{p}_{k}"] for k in ("j2d", "center", "scale")}
        compare(out, ref, pixel_bound(ref["j2d"]), f"g13 person {p}")
        np.testing.assert_allclose(out["root_aligned"], ext[f"p{p}_pose"][:, :3], rtol=R2AA_RTOL, atol=R2AA_ATOL)


def case_error_codes(be):
    joints, trans, cam_pose, K, root = make_inputs(2, seed=1)
    f64 = lambda shape: be.dev(np.zeros(shape), np.float64)
    bufs = [be.dev(joints), be.dev(trans, np.float64), be.dev(cam_pose, np.float64), be.dev(K, np.float64), be.dev(root),
            f64((2, NJ, 3)), f64((2, 2)), f64((2,)), be.zeros((2, 3))]
    call = lambda ptrs, n: be.lib.dyb_pw3d_annotate(*ptrs, n, be.stream)
    assert call([be.ptr(b) for b in bufs], 2) == 0
    for i in range(len(bufs)):
        assert call([None if j == i else be.ptr(b) for j, b in enumerate(bufs)], 2) == -1, i
    assert call([be.ptr(b) for b in bufs], 0) == -1
    assert call([be.ptr(b) for b in bufs], -3) == -1
    be.sync()


# ---------------------------------------------------------------------------------------- module level
def sequence_dict(arrays):
    """The dictionary a 3DPW sequence file unpickles to, from the arrays of golden g13 (per-person entries are lists)."""
    a = arrays
    n = a["poses"].shape[0]
    return dict(poses=[np.array(a["poses"][p]) for p in range(n)], betas=[np.array(a["betas"][p]) for p in range(n)],
                trans=[np.array(a["trans"][p]) for p in range(n)], poses2d=[np.array(a["poses2d"][p]) for p in range(n)],
                cam_poses=np.array(a["cam_poses"]), cam_intrinsics=np.array(a["cam_intrinsics"]),
                campose_valid=[np.array(a["campose_valid"][p]) for p in range(n)], genders=[str(g) for g in a["genders"]],
                sequence=str(a["sequence"]), img_frame_ids=np.array(a["img_frame_ids"]))


def smpl_pair(device):
    from dynaboa_amd import assets
    from dynaboa_amd.smpl import SMPL
    return SMPL(tables=assets.make_synthetic_smpl(MALE_SEED)).to(device), SMPL(tables=assets.make_synthetic_smpl(FEMALE_SEED)).to(device)


def extract_g13(device, out_dir, smpls, seq_idx=0, chunk=4, edit=None):
    """extract_sequence on the g13 sequence (chunk = 4 < the people's 10 and 8 frames: several chunks, the last one short)."""
    from dynaboa_amd import pw3d_extract as PX
    data = sequence_dict(golden("g13_pw3d_sequence.npz"))
    if edit is not None:
        edit(data)
    return data, PX.extract_sequence(data, seq_idx, str(out_dir), smpls[0], smpls[1], device, chunk=chunk)


def module_bounds(ext, seq, p):
    """(j3d bound, pixel bound) of person p, from the golden's own magnitudes."""
    valid = seq["campose_valid"][p].astype(bool)
    j3d = ext[f"p{p}_j3d"].astype(np.float64)
    b3 = LBS_TOL * float(np.abs(ext[f"p{p}_j3d_model"]).max()) + 2.0 ** -23 * float(np.abs(j3d).max())
    Rt = seq["cam_poses"][valid]
    z = np.einsum("nk,njk->nj", Rt[:, 2, :3], j3d) + Rt[:, None, 2, 3]
    K = seq["cam_intrinsics"]
    return b3, b3 * max(K[0, 0], K[1, 1]) / float(z.min()) + pixel_bound(ext[f"p{p}_j2d"])


def case_extract_golden(files):
    """The files of extract_g13 against golden g13.  The bounds of module_bounds come to 1.6e-4 m (person 0) / 3.0e-4 m (person 1) for
    j3d and, with f / z_min = 1969 / 3.61 and 1969 / 2.78 px per m, to 0.088 / 0.214 px for j2d, center and scale.  Measured: j3d
    1.8e-7 / 3.6e-7 m on the emulator and 1.2e-7 / 2.4e-7 m on the MI355X; j2d 9.8e-5 / 1.9e-4 px and 6.6e-5 / 1.7e-4 px; center
    3.5e-5 / 9.0e-5 and 3.4e-5 / 1.1e-4 px; scale below 1e-6 on both."""
    seq, ext = golden("g13_pw3d_sequence.npz"), golden("g13_pw3d_extract.npz")
    assert [os.path.basename(f) for f in files] == ["3dpw_0_0.npz", "3dpw_0_1.npz"]
    for p, f in enumerate(files):
        d = np.load(f)
        want = {k[3:]: ext[k] for k in ext.files if k.startswith(f"p{p}_") and k != f"p{p}_j3d_model"}
        assert sorted(d.files) == sorted(want)
        for k in d.files:
            assert d[k].dtype == want[k].dtype and d[k].shape == want[k].shape, (k, d[k].dtype, want[k].dtype, d[k].shape, want[k].shape)
        for k in ("imgname", "gender", "shape", "op_j2d"):
            assert np.array_equal(d[k], want[k]), k
        assert np.array_equal(d["pose"][:, 3:], want["pose"][:, 3:])
        np.testing.assert_allclose(d["pose"][:, :3], want["pose"][:, :3], rtol=R2AA_RTOL, atol=R2AA_ATOL)
        b3, bpx = module_bounds(ext, seq, p)
        e3 = float(np.abs(d["j3d"].astype(np.float64) - want["j3d"]).max())
        print(f"person {p}: j3d deviates by {e3:.3e} m (bound {b3:.3e})")
        assert e3 <= b3
        for k in ("j2d", "center", "scale"):
            e = float(np.abs(d[k] - want[k]).max())
            print(f"person {p}: {k} deviates by {e:.3e} (bound {bpx:.3e})")
            assert e <= bpx, (k, e, bpx)
        # the slot scatter, stated independently: BODY_25 without MidHip takes the 18 detections in order, all else stays zero
        slots = [s for s in range(19) if s != 8]
        valid = seq["campose_valid"][p].astype(bool)
        assert np.array_equal(d["op_j2d"][:, slots], seq["poses2d"][p].transpose(0, 2, 1)[valid])
        rest = [s for s in range(NJ) if s not in slots]
        assert not d["op_j2d"][:, rest].any()


def write_frames(img_dir, names):
    from PIL import Image
    for n in names:
        path = os.path.join(str(img_dir), str(n))
        os.makedirs(os.path.dirname(path), exist_ok=True)
        Image.fromarray(np.zeros((4, 4, 3), np.uint8)).save(path)


def crop_margin(kp, center, scale, d_kp, d_center, d_scale, res=224):
    """Untruncated crop coordinates of keypoints (what datasets.transform computes before ``astype(int)``) and how far a deviation of
    d_kp / d_center px and d_scale can move each: y = res * ((x - c) / h + 1 / 2) with h = 200 * scale."""
    h = 200.0 * scale
    y = res * ((kp[:, :2] - center) / h + 0.5)
    return y, res / h * (d_kp + d_center + np.abs(kp[:, :2] - center) / h * 200.0 * d_scale)


def case_round_trip(files, img_dir):
    """datasets.PW3D over the written files: length, sequences, and host_item's annotations against j2d_processing of the golden's
    arrays.  j2d_processing truncates crop coordinates to whole pixels, and the box is BUILT so that its extreme joints land exactly
    on a pixel boundary: there the last bit of centre and scale decides the pixel, and LBS is not pinned to the bit.  So: equal
    wherever the module bound on j2d / center / scale (module_bounds) cannot carry the golden's coordinate across a whole number, at
    most one crop pixel (2 / 224 after normalisation) apart elsewhere, and confidences equal.  Measured: 11 of 3528 crop
    coordinates differ on the emulator (every one a box extreme lying on a boundary) and 45 on the MI355X."""
    from dynaboa_amd import datasets as D
    seq, ext = golden("g13_pw3d_sequence.npz"), golden("g13_pw3d_extract.npz")
    ds = D.PW3D(files=list(files), img_dir=str(img_dir), device="cpu")
    n0, n1 = ext["p0_scale"].shape[0], ext["p1_scale"].shape[0]
    assert len(ds) == n0 + n1
    assert [(os.path.basename(s["file"]), s["first"], s["frames"]) for s in ds.sequences] == [("3dpw_0_0.npz", 0, n0), ("3dpw_0_1.npz", n0, n1)]
    write_frames(img_dir, ds.imgnames)
    step, moved, loose, total = 2.0 / 224.0, 0, 0, 0
    for i in range(len(ds)):
        p, r = (0, i) if i < n0 else (1, i - n0)
        h = ds.host_item(i)
        bpx = module_bounds(ext, seq, p)[1]
        c, s = ext[f"p{p}_center"][r], float(ext[f"p{p}_scale"][r])
        assert h["imgname"] == str(ext[f"p{p}_imgname"][r]) and h["gender"] == p
        assert h["frame"].shape == (4, 4, 3)
        for key, src, d_kp in (("smpl_j2d", "j2d", bpx), ("op_j2d", "op_j2d", 0.0)):
            got, want = h[key], D.j2d_processing(ext[f"p{p}_{src}"][r], c, s)
            y, margin = crop_margin(ext[f"p{p}_{src}"][r], c, s, d_kp, bpx, 2.0 * bpx / 200.0)
            firm = np.abs(y - np.round(y)) > margin
            assert np.array_equal(got[:, :2][firm], want[:, :2][firm]), (i, key)
            assert np.abs(got[:, :2] - want[:, :2]).max() <= step * (1 + 1e-6), (i, key)
            assert np.array_equal(got[:, 2], want[:, 2])
            moved, loose, total = moved + int((got != want).sum()), loose + int((~firm).sum()), total + firm.size
        assert np.array_equal(h["pose"][3:], ext[f"p{p}_pose"][r, 3:].astype("float32"))
        assert np.array_equal(h["betas"], ext[f"p{p}_shape"][r].astype("float32"))
    print(f"round trip: {moved} of {total} crop coordinates differ by one pixel ({loose} lie within the bound of a pixel boundary)")


def same_file(a, b, rows=None):
    x, y = np.load(a), np.load(b)
    assert sorted(x.files) == sorted(y.files)
    for k in x.files:
        want = y[k] if rows is None else y[k][rows]
        assert x[k].dtype == want.dtype and np.array_equal(x[k], want), k


def case_own_rules(device, tmp, smpls, full):
    """One-frame person, no-frame person, bad gender, the caller's dictionary.  `full` = the files of the unedited extraction: a frame's
    annotations depend on nothing but that frame, so the edited runs reproduce its rows exactly."""
    def one_frame(d):
        d["campose_valid"][1] = np.zeros_like(d["campose_valid"][1])
        d["campose_valid"][1][4] = 1
    data, files = extract_g13(device, tmp / "one", smpls, edit=one_frame)
    assert [os.path.basename(f) for f in files] == ["3dpw_0_0.npz", "3dpw_0_1.npz"]
    d = np.load(files[1])
    assert d["scale"].shape == (1,) and d["j3d"].shape == (1, NJ, 3) and d["pose"].shape == (1, 72) and d["imgname"].shape == (1,)
    valid1 = golden("g13_pw3d_sequence.npz")["campose_valid"][1].astype(bool)
    same_file(files[1], full[1], rows=[int(np.nonzero(np.nonzero(valid1)[0] == 4)[0][0])])
    same_file(files[0], full[0])

    def no_frame(d):
        d["campose_valid"][0] = np.zeros_like(d["campose_valid"][0])
    data, files = extract_g13(device, tmp / "none", smpls, seq_idx=5, edit=no_frame)
    assert [os.path.basename(f) for f in files] == ["3dpw_5_1.npz"] and sorted(os.listdir(tmp / "none")) == ["3dpw_5_1.npz"]
    same_file(files[0], full[1])

    def bad_gender(d):
        d["genders"][1] = "x"
    try:
        extract_g13(device, tmp / "bad", smpls, edit=bad_gender)
    except ValueError as e:
        assert "'x'" in str(e)
    else:
        raise AssertionError("a gender other than 'm' / 'f' must raise ValueError")
    assert not os.path.isdir(tmp / "bad") or not os.listdir(tmp / "bad")

    from dynaboa_amd import pw3d_extract as PX
    data = sequence_dict(golden("g13_pw3d_sequence.npz"))
    before = pickle.dumps(data, protocol=4)
    PX.extract_sequence(data, 0, str(tmp / "same"), smpls[0], smpls[1], device, chunk=64)
    assert pickle.dumps(data, protocol=4) == before
    same_file(os.path.join(str(tmp / "same"), "3dpw_0_1.npz"), full[1])           # (and the chunk size changes nothing)


def golden_dir(path):
    """The golden's two files as the reference wrote them (a directory --check can compare against)."""
    ext = golden("g13_pw3d_extract.npz")
    os.makedirs(str(path), exist_ok=True)
    for p in range(2):
        np.savez(os.path.join(str(path), f"3dpw_0_{p}.npz"),
                 **{k[3:]: ext[k] for k in ext.files if k.startswith(f"p{p}_") and k != f"p{p}_j3d_model"})


def dataset_tree(root, names, split="test"):
    """A 3DPW release holding the g13 sequence under each of `names`, every copy with its own `sequence` field."""
    d = os.path.join(str(root), "sequenceFiles", split)
    os.makedirs(d, exist_ok=True)
    for name in names:
        data = sequence_dict(golden("g13_pw3d_sequence.npz"))
        data["sequence"] = name[:-4]
        with open(os.path.join(d, name), "wb") as fh:
            pickle.dump(data, fh, protocol=2)


def case_command(device, tmp, smpls, monkeypatch, capsys):
    """python -m dynaboa_amd.pw3d_extract (its main(), in process) with --order and --check: passes against the golden's files, fails
    when one `center` of the compared directory is moved by a pixel.  Only the SMPL_*.pkl reader is replaced."""
    from dynaboa_amd import pw3d_extract as PX
    first = str(golden("g13_pw3d_sequence.npz")["sequence"]) + ".pkl"
    dataset_tree(tmp / "3dpw", [first])
    (tmp / "order.txt").write_text(first + "\n\n")
    golden_dir(tmp / "ref")
    monkeypatch.setattr(PX, "SMPL", lambda model_dir, gender="neutral", **kw: smpls[0] if gender == "male" else smpls[1])
    args = ["--pw3d_root", str(tmp / "3dpw"), "--out", str(tmp / "out"), "--order", str(tmp / "order.txt"), "--device", str(device),
            "--check", str(tmp / "ref")]
    assert PX.main(args) == 0
    text = capsys.readouterr().out
    assert "check ok" in text and "check center: largest deviation" in text and "wrote 2 files" in text
    ref1 = dict(np.load(tmp / "ref" / "3dpw_0_1.npz"))
    ref1["center"][3, 1] += 1.0
    np.savez(tmp / "ref" / "3dpw_0_1.npz", **ref1)
    assert PX.main(args) == 1
    text = capsys.readouterr().out
    assert "check failed" in text and "3dpw_0_1.npz: center" in text
    # a differing imgname or a missing key fails as well (host logic of check_files on the files just written)
    written = [str(tmp / "out" / f"3dpw_0_{p}.npz") for p in range(2)]
    golden_dir(tmp / "ref2")
    ref0 = dict(np.load(tmp / "ref2" / "3dpw_0_0.npz"))
    ref0["imgname"] = ref0["imgname"][::-1].copy()
    np.savez(tmp / "ref2" / "3dpw_0_0.npz", **ref0)
    ok, _, problems = PX.check_files(written, str(tmp / "ref2"))
    assert not ok and problems == ["3dpw_0_0.npz: imgname differs"]
    del ref0["gender"]
    np.savez(tmp / "ref2" / "3dpw_0_0.npz", **ref0)
    ok, _, problems = PX.check_files(written, str(tmp / "ref2"))
    assert not ok and "keys" in problems[0]


def case_order(device, tmp, smpls):
    """`order` decides seq_idx; a name that is not on disk raises and is named; the defaults of the two kinds of split."""
    from dynaboa_amd import constants as C, pw3d_extract as PX
    dataset_tree(tmp / "3dpw", ["a_00.pkl", "b_00.pkl"], split="validation")
    files = PX.pw3d_extract(str(tmp / "3dpw"), str(tmp / "out"), split="validation", order=["b_00.pkl", "a_00.pkl"],
                            smpl_male=smpls[0], smpl_female=smpls[1], device=device)
    assert [os.path.basename(f) for f in files] == ["3dpw_0_0.npz", "3dpw_0_1.npz", "3dpw_1_0.npz", "3dpw_1_1.npz"]
    assert str(np.load(files[0])["imgname"][0]).startswith("imageFiles/b_00/") and str(np.load(files[3])["imgname"][0]).startswith("imageFiles/a_00/")
    seq_dir = os.path.join(str(tmp / "3dpw"), "sequenceFiles", "validation")
    assert PX.sequence_order(seq_dir, "validation") == ["a_00.pkl", "b_00.pkl"]
    try:
        PX.sequence_order(seq_dir, "validation", ["a_00.pkl", "c_00.pkl"])
    except FileNotFoundError as e:
        assert "c_00.pkl" in str(e)
    else:
        raise AssertionError("a name that is not on disk must raise")
    # split='test': the table of the reference's released order.  g13's sequence carries the table's FIRST name because the
    # reference's own list begins with it (tools/make_golden_pw3d.py), so a tree holding only that file misses the second name.
    assert len(C.PW3D_TEST_ORDER) == 24 and len(set(C.PW3D_TEST_ORDER)) == 24
    first = str(golden("g13_pw3d_sequence.npz")["sequence"])
    assert C.PW3D_TEST_ORDER[0] == first
    dataset_tree(tmp / "3dpw", [first + ".pkl"], split="test")
    try:
        PX.pw3d_extract(str(tmp / "3dpw"), str(tmp / "out_test"), smpl_male=smpls[0], smpl_female=smpls[1], device=device)
    except FileNotFoundError as e:
        assert C.PW3D_TEST_ORDER[1] + ".pkl" in str(e)
    else:
        raise AssertionError("the default test order names 24 files")


def case_annotate_wrapper(device):
    """annotate() on torch tensors = the C entry (against the restatement), and it refuses wrong dtypes."""
    from dynaboa_amd import pw3d_extract as PX
    joints, trans, cam_pose, K, root = make_inputs(5, seed=11)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    out = PX.annotate(t(joints), t(trans), t(cam_pose), t(K), t(root))
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()
    ref = restate(joints, trans, cam_pose, K)
    compare({k: v.cpu().numpy() for k, v in out.items()}, ref, pixel_bound(ref["j2d"]), "annotate")
    assert out["j2d"].dtype == torch.float64 and out["root_aligned"].dtype == torch.float32 and tuple(out["scale"].shape) == (5,)
    try:
        PX.annotate(t(joints), t(trans.astype(np.float32)), t(cam_pose), t(K), t(root))
    except ValueError:
        pass
    else:
        raise AssertionError("fp32 translations must be refused")
