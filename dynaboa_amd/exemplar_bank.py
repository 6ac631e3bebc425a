"""Device-resident exemplar bank: the whole retrieval set of ``BaseAdaptor.retrieval`` (reference base_adaptor.py:82-96) kept on
the GPU, so that picking and fetching a labelled exemplar never leaves the device (csrc/retrieval.hip).

The reference takes the cluster centre nearest to ``features[5]`` by cosine distance, ``random.sample``s one member of that
cluster, decodes and crops its image on the host and uploads five small tensors - per level, per frame.  The exemplar set is small
and fixed for the whole run, so here it is preprocessed ONCE (every crop cut by the batched ``datasets.preprocess_frames``, which is
bit-identical to the single-crop entry: bank row i equals ``SourceDataset[i]`` byte for byte) and two kernels do the rest:
``dyb_retrieve_select`` (nearest centre, ties to the lowest index, and a counter-based member draw) and ``dyb_exemplar_gather`` (the
chosen rows into the stepper's exemplar inputs).

The draw rule (``--exemplar_bank 1``): member ``mulhi32(w, n_c)`` of cluster c's member list, w the first word of
``philox4x32_10(counter = (draw_lo, draw_hi, 0, 0), key = (seed_lo, seed_hi))``, ``draw`` the number of retrievals the sequence has made
so far and ``seed`` = ``options.seed``.  The sequence of exemplars then agrees with the reference's ``random.sample`` stream in
distribution, not sample by sample (the same stance as ``--teacher_dropout``).

Memory: 602 KB per exemplar, fp32 (img 3 x 224 x 224 x 4 B = 602,112 B; keypoints 588 B, pose 288 B, betas 40 B, pose_3d 384 B), plus
8 KB per cluster centre.  The reference's 10 x 10 sample set is 60 MB; uint8 / compressed storage is not implemented."""
from __future__ import annotations

import ctypes
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._abi import check
from .hmr import stream_of

FEAT = 2048
MAX_ROWS = 64                  # rows per dyb_retrieve_select call (the stepper's replica limit)
KEYS = ("img", "keypoints", "pose", "betas", "pose_3d")
_CACHE: Dict[tuple, "ExemplarBank"] = {}


def philox4x32_10(counter: Sequence[int], key: Sequence[int]) -> List[int]:
    """Philox-4x32-10 on the host (the kernels' generator, csrc/dyb_philox.h): what ``select`` will draw, for bookkeeping and tools."""
    c0, c1, c2, c3 = (int(c) & 0xffffffff for c in counter)
    k0, k1 = (int(k) & 0xffffffff for k in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & 0xffffffff, p1 & 0xffffffff, ((p0 >> 32) ^ c3 ^ k1) & 0xffffffff, p0 & 0xffffffff
        k0, k1 = (k0 + 0x9E3779B9) & 0xffffffff, (k1 + 0xBB67AE85) & 0xffffffff
    return [c0, c1, c2, c3]


def draw_member(n: int, draw: int, seed: int, sample: int = 0) -> int:
    """Position inside a cluster of n members that draw number `draw` of a sequence seeded `seed` takes."""
    w = philox4x32_10((draw & 0xffffffff, (draw >> 32) & 0xffffffff, sample, 0), (seed & 0xffffffff, (seed >> 32) & 0xffffffff))[0]
    return (w * n) >> 32


class ExemplarBank:
    """The resident tables: ``img [N][3][224][224]``, ``keypoints [N][49][3]``, ``pose [N][72]``, ``betas [N][10]``,
    ``pose_3d [N][24][4]`` (fp32, row i = ``SourceDataset[i]``), ``centers [K][2048]``, ``center_inv_norm [K]`` and the cluster
    membership as CSR (``member_ptr [K + 1]``, ``member_idx``; int32).  602 KB of device memory per exemplar."""

    def __init__(self, tables: Dict[str, torch.Tensor], imgname: Sequence[str], centers, index: Sequence[Sequence[int]], device):
        self.device = torch.device(device)
        dev = self.device
        f32 = lambda t: t.to(dev, torch.float32).contiguous()
        self.img, self.keypoints, self.pose, self.betas, self.pose_3d = (f32(tables[k]) for k in KEYS)
        self.imgname = [str(x) for x in imgname]
        N = self.items = int(self.img.shape[0])
        if tuple(self.img.shape) != (N, 3, 224, 224) or tuple(self.keypoints.shape) != (N, 49, 3) or tuple(self.pose.shape) != (N, 72) or \
                tuple(self.betas.shape) != (N, 10) or tuple(self.pose_3d.shape) != (N, 24, 4):
            raise ValueError("ExemplarBank: table shapes do not fit the exemplar item")
        c = np.ascontiguousarray(np.asarray(centers, dtype=np.float32))
        if c.ndim != 2 or c.shape[1] != FEAT or c.shape[0] != len(index) or c.shape[0] == 0:
            raise ValueError("ExemplarBank: centres must be [K][2048] with one member list per centre")
        self.clusters = int(c.shape[0])
        # torch's cosine_similarity clamps each norm at eps = 1e-8 (reference base_adaptor.py:84)
        inv = 1.0 / np.maximum(np.sqrt((c.astype(np.float64) ** 2).sum(1)), 1e-8)
        # the reference's random.sample raises on an empty cluster when it is the nearest one; on the device nobody could raise
        # inside a frame, so a cluster file with an empty cluster is refused here, where every size is known
        empty = [k for k, m in enumerate(index) if len(m) == 0]
        if empty:
            raise ValueError(f"ExemplarBank: cluster(s) {empty[:8]} have no members")
        ptr = np.zeros(self.clusters + 1, dtype=np.int32)
        ptr[1:] = np.cumsum([len(m) for m in index])
        idx = np.array([int(i) for m in index for i in m], dtype=np.int32)
        if idx.min() < 0 or idx.max() >= N:
            raise ValueError("ExemplarBank: a cluster names an exemplar outside the set")
        self.members = int(ptr[-1])
        self.index = [list(map(int, m)) for m in index]
        self.centers = torch.from_numpy(c).to(dev)
        self.center_inv_norm = torch.from_numpy(inv.astype(np.float32)).to(dev)
        self.member_ptr, self.member_idx = torch.from_numpy(ptr).to(dev), torch.from_numpy(idx).to(dev)
        self._ws = None

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.img, self.keypoints, self.pose, self.betas, self.pose_3d, self.centers,
                                                           self.center_inv_norm, self.member_ptr, self.member_idx))

    @classmethod
    def from_dataset(cls, ds, centers, index, device, workers: int = 8) -> "ExemplarBank":
        """The tables of a ``datasets.SourceDataset``: frames decoded on `workers` host threads, crops cut by the batched
        ``preprocess_frames`` (up to 64 per library call), annotations transformed by the dataset's own host arithmetic."""
        from . import datasets as D
        dev = torch.device(device)
        N = len(ds)
        img = torch.empty(N, 3, 224, 224, dtype=torch.float32, device=dev)
        with ThreadPoolExecutor(max_workers=max(1, workers)) as pool:
            for lo in range(0, N, D.CROP_MANY_MAX):
                hi = min(N, lo + D.CROP_MANY_MAX)
                frames = list(pool.map(lambda i: D.read_image(os.path.join(ds.img_dir, str(ds.imgname[i]))), range(lo, hi)))
                dfr = [torch.from_numpy(f).to(dev) for f in frames]
                D.preprocess_frames(dfr, [np.array(ds.center[i], dtype=np.float64) for i in range(lo, hi)],
                                    [float(ds.scale[i]) for i in range(lo, hi)], out=img[lo:hi])
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
        kp = np.stack([D.j2d_processing(ds.keypoints[i], np.array(ds.center[i], dtype=np.float64), float(ds.scale[i])) for i in range(N)])
        tables = dict(img=img, keypoints=f32(kp), pose=f32(ds.pose), betas=f32(ds.betas), pose_3d=f32(ds.pose_3d))
        names = [os.path.join(ds.img_dir, str(n)) for n in ds.imgname]
        return cls(tables, names, centers, index, dev)

    @classmethod
    def from_tree(cls, datapath: str, cluster_path: str, img_dir: str, device) -> "ExemplarBank":
        """The bank of a reference-style tree: `datapath` the joblib exemplar file (``h36m_random_sample_center_10_10.pt``),
        `cluster_path` the joblib cluster file ({'centers', 'index'}), `img_dir` the image root.  One bank per (files, device) is kept
        in a module cache: the adaptors of a replica group share it."""
        import joblib
        from . import datasets as D
        dev = torch.device(device)
        key = (os.path.abspath(datapath), os.path.abspath(cluster_path), os.path.abspath(img_dir), str(dev))
        hit = _CACHE.get(key)
        if hit is None:
            res = joblib.load(cluster_path)
            hit = _CACHE[key] = cls.from_dataset(D.SourceDataset(datapath, img_dir=img_dir, device=dev), np.asarray(res["centers"]),
                                                 res["index"], dev)
        return hit

    def select(self, features: torch.Tensor, draws: Sequence[int], seed: int, chunk: int = 0) -> Tuple[Dict[str, object], List[Tuple[int, int]]]:
        """The two kernels outside the stepper: features [n][2048] (or [2048]), draws[i] the draw index of row i -> (batch, picks):
        batch = the reference's retrieval dict (img [n][3][224][224], keypoints, pose, betas, pose_3d, imgname) of the chosen
        exemplars, picks[i] = (cluster, item).  Synchronises the stream (the picks come to the host)."""
        lib = _lib.load()
        x = features.detach().to(self.device, torch.float32).reshape(-1, FEAT).contiguous()
        n = int(x.shape[0])
        if n < 1 or n > MAX_ROWS or len(draws) != n:
            raise ValueError("ExemplarBank.select: 1 .. 64 feature rows and one draw index per row")
        dev = self.device
        picks = torch.full((n, 1, 2), -1, dtype=torch.int32, device=dev)
        nbytes = int(lib.dyb_retrieve_workspace_bytes(n, self.clusters, chunk))
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        rows = (ctypes.c_int * n)(*range(n))
        dr = (ctypes.c_ulonglong * MAX_ROWS)(*[int(d) & ((1 << 64) - 1) for d in draws])
        st = stream_of(x)
        asp = lambda a: ctypes.cast(a, ctypes.c_void_p)
        check(lib.dyb_retrieve_select(x.data_ptr(), FEAT * 4, asp(rows), n, self.centers.data_ptr(), self.center_inv_norm.data_ptr(),
                                      self.clusters, self.member_ptr.data_ptr(), self.member_idx.data_ptr(), self.members, self.items,
                                      asp(dr), int(seed) & ((1 << 64) - 1), 0, picks.data_ptr(), 8, 1, chunk, 1, self._ws.data_ptr(),
                                      self._ws.numel(), st), "dyb_retrieve_select")
        out = dict(img=torch.empty(n, 3, 224, 224, device=dev), keypoints=torch.empty(n, 49, 3, device=dev), pose=torch.empty(n, 72, device=dev),
                   betas=torch.empty(n, 10, device=dev), pose_3d=torch.empty(n, 24, 4, device=dev))
        dst = (ctypes.c_void_p * 5)(*[out[k].data_ptr() for k in KEYS])
        strides = (ctypes.c_size_t * 5)(*[out[k][0].numel() * 4 for k in KEYS])
        check(lib.dyb_exemplar_gather(picks.data_ptr(), 8, 1, asp(rows), n, asp(dr), self.img.data_ptr(), self.keypoints.data_ptr(),
                                      self.pose.data_ptr(), self.betas.data_ptr(), self.pose_3d.data_ptr(), self.items, asp(dst), asp(strides),
                                      st), "dyb_exemplar_gather")
        for t in out.values():
            torch.autograd.graph.increment_version(t)       # written by raw kernels
        host = [(int(c), int(i)) for c, i in picks.view(n, 2).cpu().tolist()]
        names = [self.imgname[i] for _, i in host]
        out["imgname"] = names[0] if n == 1 else names
        return out, host

    def batch_of_pick(self, pick_row: torch.Tensor) -> Dict[str, object]:
        """The retrieval dict of a logged pick ((cluster, item) row of a pick log; one small device-to-host copy)."""
        item = int(pick_row[1])
        if item < 0:
            raise RuntimeError("exemplar bank: no exemplar was picked for this draw")
        return self.batch_of([item])

    def batch_of(self, items: Sequence[int]) -> Dict[str, object]:
        """The retrieval dict of given items (views / index-selects of the tables; no kernel of the bank's own)."""
        idx = torch.tensor([int(i) for i in items], dtype=torch.long, device=self.device)
        out = {k: getattr(self, k).index_select(0, idx) for k in KEYS}
        names = [self.imgname[int(i)] for i in items]
        out["imgname"] = names[0] if len(names) == 1 else names
        return out
