"""Temporal smoothing of predicted pose sequences on the device (csrc/smooth.hip; the rules are stated in include/dynaboa_hip.h).

Every driver here adapts and infers frame by frame, so a sequence's meshes jitter; ``--seq_metrics 1`` shows it as the acceleration
error.  Two smoothers over the predicted (rotmat, beta, cam) reduce it:

  smooth_sequences   windowed and non-causal - the offline form, for written results: one ``dyb_smooth_sequences`` call over a ragged
                     batch of sequences (weighted chordal mean of the rotations, plain weighted mean of the other channels), never
                     across a sequence end, an invalid frame or a gap in the frame numbers;
  OneEuro            causal - the live form: one ``dyb_one_euro_step`` launch per step for all the sequences it filters.

``smooth_results`` is the pass over the ``result/Pred_{n}.pt`` dumps of a finished run (-> ``result_smooth/``), and

    python -m dynaboa_amd.smooth --expdir D --expname N --half_window H [--sigma S]

is the 3DPW pass over the dumps of a ``--dump_predictions 1`` run: the 14 joints of the raw and of the smoothed parameters against the
dataset's ground truth through two ``sequence_metrics_device`` calls -> ``metrics_smoothed.json``,
``metrics_per_sequence_smoothed.csv`` and one ``ACCEL: raw -> smoothed`` line.  The reference has no smoother."""
from __future__ import annotations

import argparse
import copy
import json
import os
from typing import Callable, List, Optional, Sequence, Union

import numpy as np
import torch

MAX_HALF_WINDOW = 32               # DYB_SMOOTH_MAX_HALF_WINDOW
SMPL_CHUNK = 1024                  # frames per SMPL forward of the passes over dumps
SMOOTH_CHUNK = 65536               # frames per dyb_smooth_sequences call of the passes (whole sequences; a longer one goes alone)


def gaussian_weights(half_window: int, sigma: Optional[float] = None) -> np.ndarray:
    """exp(-k^2 / (2 sigma^2)) for k = -half_window .. half_window, computed in float64 and rounded once to float32; sigma defaults
    to half_window / 2.  (The kernel divides by the sum of the taps it uses: no normalisation here.)"""
    h = int(half_window)
    if not 0 <= h <= MAX_HALF_WINDOW:
        raise ValueError(f"half_window {half_window} outside 0..{MAX_HALF_WINDOW}")
    if h == 0:
        return np.ones(1, np.float32)
    sigma = h / 2.0 if sigma is None else float(sigma)
    if not sigma > 0:
        raise ValueError(f"sigma {sigma} must be positive")
    k = np.arange(-h, h + 1, dtype=np.float64)
    return np.exp(-0.5 * (k / sigma) ** 2).astype(np.float32)


def _ptr(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def smooth_sequences(rotmat: torch.Tensor, betas: Optional[torch.Tensor] = None, cam: Optional[torch.Tensor] = None, *, lengths,
                     valid=None, frame_id=None, half_window: int = 4, sigma: Optional[float] = None, weights=None):
    """rotmat (n, J, 3, 3) or (n, J, 9), betas (n, nb) and cam (n, nc) optional: device tensors, the frames of len(lengths) sequences
    one after the other (the conventions of ``pose_utils.sequence_metrics_device``: lengths are ints summing to n, zeros allowed;
    valid (n,) bool and frame_id (n,) int tensors optional).  weights: 2 half_window + 1 tap weights (default:
    ``gaussian_weights(half_window, sigma)``).  -> (rotmat, betas, cam) smoothed, new device tensors of the inputs' shapes (None where
    None was given).  One dyb_smooth_sequences call on rotmat's stream; nothing is copied to the host."""
    from . import _lib
    from ._abi import check
    from .hmr import stream_of
    shape = rotmat.shape
    n, J = int(shape[0]), int(shape[1])
    rot = rotmat.contiguous().float().reshape(n, J, 9)
    lengths = [int(v) for v in lengths]
    if not lengths or min(lengths) < 0 or sum(lengths) != n:
        raise ValueError(f"sequence lengths {lengths} do not tile {n} frames")
    h = int(half_window)
    w = np.ascontiguousarray(gaussian_weights(h, sigma) if weights is None else np.asarray(weights, np.float32))
    if w.shape != (2 * h + 1,):
        raise ValueError(f"{w.size} weights for half_window {h}: {2 * h + 1} expected")
    dev = rot.device
    chan = lambda t: None if t is None else t.to(dev).contiguous().float().reshape(n, int(np.prod(t.shape[1:])))
    b, c = chan(betas), chan(cam)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int32).to(dev)
    if valid is not None:
        valid = valid.to(dev).reshape(n).to(torch.uint8).contiguous()
    if frame_id is not None:
        frame_id = frame_id.to(dev).reshape(n).to(torch.int32).contiguous()
    out_r = torch.empty_like(rot)
    out_b = None if b is None else torch.empty_like(b)
    out_c = None if c is None else torch.empty_like(c)
    check(_lib.load().dyb_smooth_sequences(_ptr(rot), _ptr(b), 0 if b is None else int(b.shape[1]), _ptr(c), 0 if c is None else int(c.shape[1]),
                                           offsets.data_ptr(), len(lengths), _ptr(valid), _ptr(frame_id), w.ctypes.data, h, _ptr(out_r),
                                           _ptr(out_b), _ptr(out_c), n, J, stream_of(rot)), "dyb_smooth_sequences")
    return (out_r.reshape(shape), None if betas is None else out_b.reshape(betas.shape), None if cam is None else out_c.reshape(cam.shape))


class OneEuro:
    """The One-Euro filter (Casiez et al. 2012) over the pose of `n_seq` sequences at once: per joint a quaternion, per beta and
    camera channel a scalar (the groups and the update are stated at dyb_one_euro_step).  ``step`` is one launch whatever n_seq is.
    The state is ONE device tensor, ``self.state`` (n_seq, dyb_one_euro_state_floats(J, nb, nc)); a zeroed row is a filter that has
    not started: its first step returns its input."""

    def __init__(self, n_seq: int, fps: float = 30.0, min_cutoff: float = 1.0, beta: float = 0.0, d_cutoff: float = 1.0, J: int = 24,
                 nb: int = 10, nc: int = 3, device="cuda"):
        from . import _lib
        if n_seq < 1 or not fps > 0 or not min_cutoff > 0 or not d_cutoff > 0 or beta < 0:
            raise ValueError("OneEuro: n_seq >= 1, fps > 0, min_cutoff > 0, d_cutoff > 0 and beta >= 0 are required")
        self.n_seq, self.J, self.nb, self.nc = int(n_seq), int(J), int(nb), int(nc)
        self.te, self.min_cutoff, self.beta, self.d_cutoff = 1.0 / float(fps), float(min_cutoff), float(beta), float(d_cutoff)
        floats = _lib.load().dyb_one_euro_state_floats(self.J, self.nb, self.nc)
        if floats <= 0:
            raise ValueError(f"OneEuro: bad sizes J {J}, nb {nb}, nc {nc}")
        self.device = torch.device(device)
        self.state = torch.zeros(self.n_seq, floats, dtype=torch.float32, device=self.device)

    def reset(self, seq=None):
        """Forget the past of sequence `seq` (an index or a list of them; None: of all): its next step returns its input."""
        if seq is None:
            self.state.zero_()
        else:
            self.state[seq] = 0

    def step(self, rotmat: torch.Tensor, betas: torch.Tensor, cam: torch.Tensor, active=None):
        """rotmat (n_seq, J, 3, 3) or (n_seq, J, 9), betas (n_seq, nb), cam (n_seq, nc) -> the filtered three, new tensors.  active
        (n_seq,) bools (a tensor or a list; None: all): an inactive sequence's state is not touched and its output rows are its
        input rows."""
        from . import _lib
        from ._abi import check
        from .hmr import stream_of
        R = self.n_seq
        shape = rotmat.shape
        rot = rotmat.to(self.device).contiguous().float().reshape(R, self.J, 9)
        b = betas.to(self.device).contiguous().float().reshape(R, self.nb)
        c = cam.to(self.device).contiguous().float().reshape(R, self.nc)
        if active is not None:
            active = torch.as_tensor(active).to(self.device).reshape(R).to(torch.uint8).contiguous()
        # an inactive row is not written by the kernel: start from the inputs
        out_r, out_b, out_c = (rot.clone(), b.clone(), c.clone()) if active is not None else (torch.empty_like(rot), torch.empty_like(b), torch.empty_like(c))
        check(_lib.load().dyb_one_euro_step(self.state.data_ptr(), _ptr(rot), _ptr(b), self.nb, _ptr(c), self.nc, _ptr(active), self.te,
                                            self.min_cutoff, self.beta, self.d_cutoff, _ptr(out_r), _ptr(out_b), _ptr(out_c), R, self.J,
                                            stream_of(rot)), "dyb_one_euro_step")
        return out_r.reshape(shape), out_b.reshape(betas.shape), out_c.reshape(cam.shape)


# ------------------------------------------------------------------------------------------------------ the pass over written dumps
def _load_dumps(exppath: str, rows: Sequence[int], src: str):
    import joblib
    dumps = []
    for n in rows:
        path = os.path.join(exppath, src, f"Pred_{n}.pt")
        if not os.path.isfile(path):
            raise FileNotFoundError(f"smoothing: row {n} has no {path}")
        d = joblib.load(path)
        if np.asarray(d["rotmat"]).reshape(-1, 24, 9).shape[0] != 1:
            raise ValueError(f"{path} holds a batch of {np.asarray(d['rotmat']).reshape(-1, 24, 9).shape[0]}: the smoothing pass reads "
                             "the dumps of a batch-size-1 run (one frame per file)")
        dumps.append(d)
    return dumps


def smpl_vertices(smpl, rotmat: torch.Tensor, betas: torch.Tensor, chunk: int = SMPL_CHUNK) -> torch.Tensor:
    """SMPL forward of (n, 24, 3, 3) rotations and (n, 10) betas in chunks of at most `chunk` frames -> vertices (n, 6890, 3)."""
    out = []
    with torch.no_grad():
        for lo in range(0, int(rotmat.shape[0]), chunk):
            r, b = rotmat[lo:lo + chunk], betas[lo:lo + chunk]
            out.append(smpl(betas=b, body_pose=r[:, 1:], global_orient=r[:, 0].unsqueeze(1), pose2rot=False).vertices)
    return torch.cat(out) if out else torch.zeros(0, 6890, 3, device=rotmat.device)


def smooth_results(exppath: str, sequences: Sequence[Sequence[int]], smpl, *, half_window: int, sigma: Optional[float] = None,
                   frame_ids: Optional[Sequence[Sequence[int]]] = None,
                   cam_frame: Union[None, np.ndarray, Callable[[int, dict], np.ndarray]] = None, src: str = "result",
                   dst: str = "result_smooth") -> List[str]:
    """The windowed smoother over the dumps of a finished batch-size-1 run.  `sequences`: a list of row lists; row n names
    ``<exppath>/<src>/Pred_{n}.pt`` (a missing file raises FileNotFoundError naming it).  frame_ids: per sequence the rows' frame
    numbers (None: consecutive).  One ``smooth_sequences`` call per chunk of whole sequences, then SMPL forward (`smpl`: the neutral
    ``SMPL`` module, on the device the pass runs on) in chunks of at most 1024 frames, then ``<exppath>/<dst>/Pred_{n}.pt`` with the
    source's keys: ``verts``, ``rotmat`` and ``beta`` smoothed, ``cam`` the frame's own value, untouched - the crop camera belongs to
    that frame's box, and the box jitters too.  cam_frame: the full-frame camera (sx, sy, tx, ty) of every row - an (n, 4) array in the
    order of the rows of `sequences`, or a function (row, dump) -> (4,); its smoothed value is written as a further key
    ``cam_frame``.  -> the written paths."""
    import joblib
    sequences = [[int(n) for n in s] for s in sequences]
    if frame_ids is not None and [len(f) for f in frame_ids] != [len(s) for s in sequences]:
        raise ValueError("frame_ids must list one id per row of every sequence")
    dev = next(smpl.buffers()).device
    os.makedirs(os.path.join(exppath, dst), exist_ok=True)
    paths, first = [], 0
    ids = None if frame_ids is None else list(frame_ids)
    for chunk in _chunk_indices(sequences):
        rows = [n for si in chunk for n in sequences[si]]
        dumps = _load_dumps(exppath, rows, src)
        if not rows:
            continue
        rot = torch.from_numpy(np.stack([np.asarray(d["rotmat"], np.float32).reshape(24, 9) for d in dumps])).to(dev)
        beta = torch.from_numpy(np.stack([np.asarray(d["beta"], np.float32).reshape(-1) for d in dumps])).to(dev)
        camf = None
        if cam_frame is not None:
            if callable(cam_frame):
                camf = np.stack([np.asarray(cam_frame(n, d), np.float32).reshape(4) for n, d in zip(rows, dumps)])
            else:
                camf = np.asarray(cam_frame, np.float32).reshape(-1, 4)[first:first + len(rows)]
            camf = torch.from_numpy(np.ascontiguousarray(camf)).to(dev)
        fid = None if ids is None else torch.tensor([int(v) for si in chunk for v in ids[si]], dtype=torch.int32)
        s_rot, s_beta, s_cam = smooth_sequences(rot, beta, camf, lengths=[len(sequences[si]) for si in chunk], frame_id=fid,
                                                half_window=half_window, sigma=sigma)
        verts = smpl_vertices(smpl, s_rot.reshape(-1, 24, 3, 3), s_beta).cpu().numpy()
        s_rot, s_beta = s_rot.cpu().numpy(), s_beta.cpu().numpy()
        s_cam = None if s_cam is None else s_cam.cpu().numpy()
        for k, (n, d) in enumerate(zip(rows, dumps)):
            out = dict(d)
            out["verts"] = verts[k].reshape(np.shape(d["verts"])).astype(np.asarray(d["verts"]).dtype)
            out["rotmat"] = s_rot[k].reshape(np.shape(d["rotmat"])).astype(np.asarray(d["rotmat"]).dtype)
            out["beta"] = s_beta[k].reshape(np.shape(d["beta"])).astype(np.asarray(d["beta"]).dtype)
            if s_cam is not None:
                out["cam_frame"] = s_cam[k].copy()
            path = os.path.join(exppath, dst, f"Pred_{n}.pt")
            joblib.dump(out, path)
            paths.append(path)
        first += len(rows)
    return paths


def _chunk_indices(sequences, limit=None):
    """Indices of whole sequences, as many as fit under `limit` (default SMOOTH_CHUNK) frames per chunk; a longer sequence is a chunk
    of its own."""
    limit = SMOOTH_CHUNK if limit is None else limit
    chunk, frames = [], 0
    for si, s in enumerate(sequences):
        if chunk and frames + len(s) > limit:
            yield chunk
            chunk, frames = [], 0
        chunk.append(si)
        frames += len(s)
    if chunk:
        yield chunk


# ------------------------------------------------------------------------------------------------------ 3DPW: the pass with metrics
def regress14(verts: torch.Tensor, J_regressor: torch.Tensor, joint_mapper: Sequence[int]) -> torch.Tensor:
    """The 14 evaluation joints of vertices (n, 6890, 3), root-aligned, exactly as ``benchmark.Adaptor._regress14`` forms them:
    dyb_regress_joints with the H36M regressor (17 joints), the mapper's 14 of them, minus joint 0."""
    from . import _lib
    from ._abi import check
    from .hmr import stream_of
    v = verts.contiguous().float()
    reg = J_regressor.to(v.device).contiguous().float()
    out = torch.empty(int(v.shape[0]), 17, 3, dtype=torch.float32, device=v.device)
    if v.shape[0]:
        check(_lib.load().dyb_regress_joints(reg.data_ptr(), v.data_ptr(), out.data_ptr(), 17, int(v.shape[0]), stream_of(v)),
              "dyb_regress_joints")
    idx = torch.tensor(list(joint_mapper), dtype=torch.long, device=v.device)
    return out.index_select(1, idx) - out[:, 0:1, :]


def gt14_of(pose: torch.Tensor, betas: torch.Tensor, gender: torch.Tensor, smpl_male, smpl_female, J_regressor, joint_mapper,
            chunk: int = SMPL_CHUNK) -> torch.Tensor:
    """The ground-truth 14 joints as ``benchmark.Adaptor.inference`` forms ``gt14``: the male and the female model on the axis-angle
    pose (n, 72) and betas (n, 10), the female vertices where gender == 1, through ``regress14``."""
    out = []
    with torch.no_grad():
        for lo in range(0, int(pose.shape[0]), chunk):
            p, b, g = pose[lo:lo + chunk], betas[lo:lo + chunk], gender[lo:lo + chunk]
            vm = smpl_male(global_orient=p[:, :3], body_pose=p[:, 3:], betas=b).vertices
            vf = smpl_female(global_orient=p[:, :3], body_pose=p[:, 3:], betas=b).vertices
            out.append(regress14(torch.where((g == 1).view(-1, 1, 1), vf, vm), J_regressor, joint_mapper))
    return torch.cat(out) if out else torch.zeros(0, 14, 3, device=pose.device)


def _report_block(frame: np.ndarray, seq: np.ndarray, names):
    """One block of metrics_smoothed.json, shaped like ``benchmark.sequence_summary``'s pair (no PVE: the pass forms joints only)."""
    from . import benchmark as DB, pose_utils as PU
    rows = [DB.sequence_row(nm, seq[j]) for j, nm in enumerate(names)]
    res = dict(mpjpe=frame[:, PU.FRAME_MPJPE] * 1000, pampjpe=frame[:, PU.FRAME_PAMPJPE] * 1000, pve=np.zeros(0),
               accel=frame[:, PU.FRAME_ACCEL] * 1000, accel_counted=frame[:, PU.FRAME_ACCEL_COUNTED] > 0.5, pck=frame[:, PU.FRAME_PCK],
               auc=frame[:, PU.FRAME_AUC], per_sequence=rows)
    overall, seq_mean = DB.sequence_summary(res)
    overall.pop("pve", None)
    return dict(overall=overall, sequence_mean=seq_mean), rows


def smooth_metrics(exppath: str, sequences: Sequence[Sequence[int]], names: Sequence[str], pose, betas, gender, smpl_neutral, smpl_male,
                   smpl_female, J_regressor, joint_mapper, *, half_window: int, sigma: Optional[float] = None,
                   frame_ids: Optional[Sequence[Sequence[int]]] = None, src: str = "result") -> dict:
    """The 3DPW pass.  `sequences`: row lists, row n names ``<src>/Pred_{n}.pt`` of a batch-size-1 ``--dump_predictions 1`` run and
    row n of the ground-truth columns pose (N, 72), betas (N, 10), gender (N,).  The raw and the smoothed parameters go through SMPL
    and ``regress14``, the ground truth through ``gt14_of``; two ``sequence_metrics_device`` calls -> ``metrics_smoothed.json``
    (blocks ``raw`` and ``smoothed``), ``metrics_per_sequence_smoothed.csv`` (one line per sequence: the smoothed row's columns and
    the raw acceleration error, worst smoothed PA-MPJPE first) under `exppath`.  -> dict(raw=, smoothed=) of the two blocks."""
    from . import pose_utils as PU
    sequences = [[int(n) for n in s] for s in sequences]
    dev = next(smpl_neutral.buffers()).device
    rows = [n for s in sequences for n in s]
    lengths = [len(s) for s in sequences]
    dumps = _load_dumps(exppath, rows, src)
    if rows:
        rot = torch.from_numpy(np.stack([np.asarray(d["rotmat"], np.float32).reshape(24, 3, 3) for d in dumps])).to(dev)
        beta = torch.from_numpy(np.stack([np.asarray(d["beta"], np.float32).reshape(-1) for d in dumps])).to(dev)
    else:
        rot, beta = torch.zeros(0, 24, 3, 3, device=dev), torch.zeros(0, 10, device=dev)
    fid = None if frame_ids is None else torch.tensor([int(v) for f in frame_ids for v in f], dtype=torch.int32)
    s_rot, s_beta, _ = smooth_sequences(rot, beta, lengths=lengths, frame_id=fid, half_window=half_window, sigma=sigma)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a)[rows])).to(dev).to(dt)
    gt14 = gt14_of(t(pose, torch.float32), t(betas, torch.float32), t(gender, torch.long), smpl_male, smpl_female, J_regressor, joint_mapper)
    blocks, per_seq = {}, {}
    for key, (r, b) in (("raw", (rot, beta)), ("smoothed", (s_rot, s_beta))):
        pred14 = regress14(smpl_vertices(smpl_neutral, r, b), J_regressor, joint_mapper)
        frame, seq = PU.sequence_metrics_device(pred14, gt14, lengths, frame_id=fid)
        blocks[key], per_seq[key] = _report_block(frame.cpu().numpy(), seq.cpu().numpy(), names)
    os.makedirs(exppath, exist_ok=True)
    with open(os.path.join(exppath, "metrics_smoothed.json"), "w") as f:
        json.dump(dict(half_window=int(half_window), sigma=sigma, sequences=len(sequences), **blocks), f, indent=1)
    cols = ("name", "frames", "mpjpe", "pampjpe", "pck", "auc", "accel", "triples")
    with open(os.path.join(exppath, "metrics_per_sequence_smoothed.csv"), "w") as f:
        f.write(",".join(cols + ("accel_raw", "mpjpe_raw", "pampjpe_raw")) + "\n")
        raw_of = {r["name"]: r for r in per_seq["raw"]}
        for r in sorted(per_seq["smoothed"], key=lambda r: -r["pampjpe"]):
            q = raw_of[r["name"]]
            f.write(",".join([str(r[c]) for c in cols] + [str(q["accel"]), str(q["mpjpe"]), str(q["pampjpe"])]) + "\n")
    return blocks


def smoothed_line(blocks: dict) -> str:
    raw, sm = blocks["raw"]["overall"], blocks["smoothed"]["overall"]
    return (f"ACCEL: {raw['accel']} -> {sm['accel']}, MPJPE: {raw['mpjpe']} -> {sm['mpjpe']}, "
            f"PAMPJPE: {raw['pampjpe']} -> {sm['pampjpe']}")


def _make_parser():
    """The benchmark driver's parser, copied as the internet driver copies it (the run's own flags locate its dataset and files),
    plus the pass's own."""
    from . import benchmark as DB
    p = copy.deepcopy(DB.parser)
    p.description = __doc__
    p.formatter_class = argparse.RawDescriptionHelpFormatter
    p.add_argument('--half_window', type=int, default=4, help=f'taps on either side of a frame, 0..{MAX_HALF_WINDOW} (0: no smoothing)')
    p.add_argument('--sigma', type=float, default=None, help='of the Gaussian weights, in frames (default: half_window / 2)')
    p.add_argument('--write_results', type=int, default=0, choices=[0, 1], help='1: also write result_smooth/Pred_{n}.pt')
    return p


def run_pw3d(options, device=None):
    """The pass over ``<expdir>/<expname>/result`` of a finished 3DPW run: the dataset's sequences and ground-truth columns (the
    files ``benchmark.Adaptor`` reads them from), frame ids from the image names."""
    from . import benchmark as DB, constants, datasets as D
    from .smpl import SMPL
    if int(getattr(options, "batch_size", 1)) != 1:
        raise ValueError("the smoothing pass reads the dumps of a batch-size-1 run (Pred_{n}.pt = frame n): --batch_size 1")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    ds = D.PW3D(None, img_dir=getattr(options, "pw3d_root", None) or D.PW3D_ROOT, device=dev)
    smpl = {g: SMPL("data/smpl", create_transl=False, **({} if g == "neutral" else {"gender": g})).to(dev) for g in ("neutral", "male", "female")}
    J_regressor = torch.from_numpy(np.load("data/J_regressor_h36m.npy")).float()
    exppath = os.path.join(options.expdir, options.expname)
    sequences = [list(range(s["first"], s["first"] + s["frames"])) for s in ds.sequences]
    names = [os.path.splitext(os.path.basename(str(s["file"])))[0] for s in ds.sequences]
    ids = [DB._frame_ids([ds.imgnames[n] for n in s], len(s)) for s in sequences]
    ids = None if any(x is None for x in ids) else ids
    blocks = smooth_metrics(exppath, sequences, names, ds.pose, ds.betas, ds.genders, smpl["neutral"], smpl["male"], smpl["female"],
                            J_regressor, list(constants.H36M_TO_J14), half_window=options.half_window, sigma=options.sigma, frame_ids=ids)
    if getattr(options, "write_results", 0):
        smooth_results(exppath, sequences, smpl["neutral"], half_window=options.half_window, sigma=options.sigma, frame_ids=ids)
    print(smoothed_line(blocks))
    return blocks


def main(argv=None):
    return run_pw3d(_make_parser().parse_args(argv))


if __name__ == '__main__':
    main()
