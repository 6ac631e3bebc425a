"""Build the exemplar retrieval index on the device: the three files under ``data/retrieval_res/`` that ``--retrieval 1`` and
``--exemplar_bank 1`` read (reference base_adaptor.py:55, 74-80), from a labelled source set and ANY checkpoint.

The reference ships those files as a download and has no code that makes them; the procedure here is this project's own:

1. ``extract_features``: ``features[5]`` (the pooled 2048-vector) of every source row, crops cut by ``datasets.preprocess_frames``.
2. ``kmeans``: spherical k-means, a host-driven Lloyd loop over three kernels of csrc/kmeans.hip (row norms, assignment on the exact
   fp32 matrix cores with a fused argmax, a deterministic centre update without floating-point atomics).
3. ``select_members``: a seeded draw (or the nearest rows) of ``per_cluster`` exemplars per cluster.
4. ``build_index`` / ``python -m dynaboa_amd.retrieval_index``: the files, under the reference's names.

Random numbers are words of ``exemplar_bank.philox4x32_10`` (the kernels' generator) under key ``(seed & 0xffffffff, seed >> 32)``:

* k-means initial centres (``init=None``): a partial Fisher-Yates over the row indices 0 .. N - 1.  Draw j = 0 .. K - 1 takes
  ``w = philox4x32_10(counter = (j, 0, 0, 1), key)[0]``, ``r = j + mulhi32(w, N - j)`` and swaps positions j and r; the initial
  centres are the rows at positions 0 .. K - 1, K distinct rows.
* ``select_members(mode="random")``: cluster k's ascending member list m of n rows, draw j = 0 .. min(per_cluster, n) - 1 takes
  ``w = philox4x32_10(counter = (j, 0, k, 2), key)[0]``, ``r = j + mulhi32(w, n - j)`` and swaps m[j] and m[r]; the kept rows are
  m[0 .. min(per_cluster, n) - 1] in draw order.

``mulhi32(w, n) = (w * n) >> 32``.  Word 3 of the counter tells the streams apart from the exemplar bank's member draw (word 3 = 0)."""
from __future__ import annotations

import argparse
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._abi import check
from .exemplar_bank import FEAT, philox4x32_10

SAMPLE_FILE = "h36m_random_sample_center_10_10.pt"                       # reference base_adaptor.py:55
CLUSTER_FILE = "cluster_res_random_sample_center_10_10_potocol2.pt"      # reference base_adaptor.py:76
FEATS_FILE = "h36m_feats_random_sample_center_10_10.pt"
SOURCE_KEYS = ("imgname", "scale", "center", "pose", "shape", "S", "part")
MAX_K = 1024


def _key(seed: int) -> Tuple[int, int]:
    return int(seed) & 0xffffffff, (int(seed) >> 32) & 0xffffffff


def init_rows(N: int, K: int, seed: int) -> List[int]:
    """The K distinct rows ``kmeans(init=None)`` starts from (the module docstring's rule)."""
    if not 1 <= K <= N:
        raise ValueError("kmeans: need 1 <= K <= N")
    pos: Dict[int, int] = {}
    key = _key(seed)
    out = []
    for j in range(K):
        w = philox4x32_10((j, 0, 0, 1), key)[0]
        r = j + ((w * (N - j)) >> 32)
        vj, vr = pos.get(j, j), pos.get(r, r)
        pos[j], pos[r] = vr, vj
        out.append(vr)
    return out


# ------------------------------------------------------------------------------------------------------------------ Lloyd loop
class DeviceOps:
    """The device side of one k-means run over a fixed feature matrix: buffers and the three library calls.  ``alloc(shape, dtype)``
    -> a zeroed buffer, ``ptr(buf)`` -> its address, ``to_host(buf)`` -> ndarray (after the stream's work), ``upload(buf, ndarray)``;
    the torch form below and the tests' form over a kernel backend differ only in these four."""

    def __init__(self, lib, stream, x, x_stride_bytes: int, N: int, D: int, K: int, alloc, ptr, to_host, upload):
        if not (N >= 1 and D % 32 == 0 and 1 <= K <= MAX_K):
            raise ValueError("kmeans: N >= 1, D a multiple of 32 and 1 <= K <= 1024")
        self.lib, self.stream, self.x, self.stride, self.N, self.D, self.K = lib, stream, x, int(x_stride_bytes), N, D, K
        self.ptr, self.to_host, self.upload = ptr, to_host, upload
        self.x_inv = alloc((N,), np.float32)
        self.centers = alloc((K, D), np.float32)
        self.c_inv = alloc((K,), np.float32)
        self.assign = alloc((N,), np.int32)
        self.best = alloc((N,), np.float32)
        # one buffer for the small per-iteration read: changed | counts [K] | (pad to 8 bytes) | fp64 objective partials
        self.ntiles = int(lib.dyb_kmeans_assign_workspace_bytes(N, D, K)) // 8
        self.head = (1 + K + 1) // 2 * 2
        self.small = alloc((self.head + 2 * self.ntiles,), np.int32)
        self.up_bytes = int(lib.dyb_kmeans_update_workspace_bytes(N, D, K))
        self.up_ws = alloc((self.up_bytes // 4,), np.float32)
        check(lib.dyb_rows_inv_norm(ptr(x), self.stride, N, D, ptr(self.x_inv), stream), "dyb_rows_inv_norm")

    def start(self, centers: np.ndarray):
        self.upload(self.centers, np.ascontiguousarray(centers, dtype=np.float32).reshape(self.K, self.D))
        self.upload(self.assign, np.full(self.N, -1, np.int32))

    def assign_step(self) -> Tuple[int, np.ndarray, float]:
        """centre norms, the assignment, and the one small read -> (changed, counts [K], objective = sum of best)"""
        lib, p, K = self.lib, self.ptr, self.K
        check(lib.dyb_rows_inv_norm(p(self.centers), self.D * 4, K, self.D, p(self.c_inv), self.stream), "dyb_rows_inv_norm")
        base = p(self.small)
        check(lib.dyb_kmeans_assign(p(self.x), self.stride, p(self.x_inv), self.N, self.D, p(self.centers), p(self.c_inv), K, p(self.assign),
                                    p(self.best), base, base + 4, base + 4 * self.head, 8 * self.ntiles, self.stream), "dyb_kmeans_assign")
        small = self.to_host(self.small)
        parts = small[self.head:].view(np.float64)
        obj = 0.0
        for v in parts:                                   # in index order
            obj += float(v)
        return int(small[0]), small[1:1 + K].astype(np.int64), obj

    def update(self, counts: np.ndarray):
        lib, p = self.lib, self.ptr
        self.upload(self.small[1:1 + self.K], np.asarray(counts, dtype=np.int32))
        check(lib.dyb_kmeans_update(p(self.x), self.stride, p(self.x_inv), self.N, self.D, p(self.assign), p(self.small) + 4, self.K,
                                    p(self.centers), p(self.up_ws), self.up_bytes, self.stream), "dyb_kmeans_update")


def lloyd(ops: DeviceOps, init: np.ndarray, max_iter: int = 100, trace: Optional[list] = None):
    """Assign, one small read, (reseed of empty clusters,) update - until no assignment changes or max_iter assigns were made.

    Empty clusters (after an assign, before the update), in ascending cluster index: the cluster takes the row with the lowest
    ``best`` (ties: the lowest row index) that has not been taken in this iteration and is not the only member of its cluster; the
    row is reassigned, both counts corrected, and the update makes it the centre.  ``best`` comes to the host only then.
    -> (centers [K][D] ndarray, assign [N] ndarray, info).  `trace`, if given, receives a copy of the assignment after every
    iteration's reseeds (tests)."""
    ops.start(init)
    info = dict(iterations=0, objective=[], reseeds=0)
    for _ in range(max(1, int(max_iter))):
        changed, counts, obj = ops.assign_step()
        info["iterations"] += 1
        info["objective"].append(obj)
        empty = [k for k in range(ops.K) if counts[k] == 0]
        if empty:
            best = ops.to_host(ops.best).astype(np.float64)
            assign = ops.to_host(ops.assign).copy()
            order = np.lexsort((np.arange(ops.N), best))              # lowest best first, ties to the lowest row
            at = 0
            for k in empty:
                while at < ops.N and counts[assign[order[at]]] <= 1:
                    at += 1
                if at >= ops.N:
                    break                                             # fewer spare rows than empty clusters: they stay empty
                row = int(order[at])
                at += 1
                counts[assign[row]] -= 1
                assign[row] = k
                counts[k] = 1
                info["reseeds"] += 1
            ops.upload(ops.assign, assign)
        if trace is not None:
            trace.append(ops.to_host(ops.assign).copy())
        if changed == 0 and not empty:
            break
        ops.update(counts)
    info["best"] = ops.to_host(ops.best).copy()           # the winning cosines of the last assign (a reseeded row: before its reseed)
    return ops.to_host(ops.centers).copy(), ops.to_host(ops.assign).copy(), info


def _torch_ops(features: torch.Tensor, K: int) -> DeviceOps:
    from . import _lib
    from .hmr import stream_of
    x = features.detach()
    if x.dim() != 2 or x.dtype != torch.float32 or x.stride(1) != 1 or (x.stride(0) * 4) % 16 or x.data_ptr() % 16:
        x = x.to(torch.float32).contiguous()
    dev = x.device
    td = {np.float32: torch.float32, np.int32: torch.int32}

    def to_host(b):
        return b.cpu().numpy()                            # (waits for the stream's work)

    def upload(b, a):
        b.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dev))

    return DeviceOps(_lib.load(), stream_of(x), x, x.stride(0) * 4, int(x.shape[0]), int(x.shape[1]), int(K),
                     lambda s, d: torch.zeros(s, dtype=td[d], device=dev), lambda b: b.data_ptr(), to_host, upload)


def kmeans(features: torch.Tensor, K: int, seed: int, init=None, max_iter: int = 100, n_init: int = 1):
    """Spherical k-means of ``features`` [N][D] (fp32, on the device; D a multiple of 32, K <= 1024) -> (centers [K][D] device tensor,
    un-normalised means of the unit rows; assign [N] int32 device tensor; info = {'iterations', 'objective' (sum of the winning
    cosines at every assign), 'reseeds', 'seed', 'best' (the last assign's winning cosines, [N] ndarray)}).  ``init``: explicit centres [K][D], or None for K distinct rows drawn by the
    module docstring's Philox rule under ``seed``.  ``n_init`` > 1 (init None) runs seeds seed, seed + 1, ... and keeps the run with
    the highest final objective, the first on a tie.  Rules of the loop: ``lloyd``."""
    ops = _torch_ops(features, K)
    best = None
    runs = 1 if init is not None else max(1, int(n_init))
    for r in range(runs):
        if init is not None:
            c0 = init.detach().cpu().numpy() if torch.is_tensor(init) else np.asarray(init)
        else:
            rows = torch.tensor(init_rows(ops.N, K, seed + r), dtype=torch.long, device=ops.x.device)
            c0 = ops.x.index_select(0, rows)[:, :ops.D].cpu().numpy()
        centers, assign, info = lloyd(ops, c0, max_iter)
        info["seed"] = seed + r
        if best is None or info["objective"][-1] > best[2]["objective"][-1]:
            best = (centers, assign, info)
    dev = ops.x.device
    return torch.from_numpy(best[0]).to(dev), torch.from_numpy(best[1]).to(dev), best[2]


# ------------------------------------------------------------------------------------------------------------------ member draw
def select_members(assign, K: int, per_cluster: int, seed: int, best=None, mode: str = "random") -> List[List[int]]:
    """Rows kept per cluster (host).  random: the module docstring's seeded partial Fisher-Yates over the cluster's ascending member
    list; nearest: the rows of highest ``best``, ties to the lowest row.  A cluster of fewer than per_cluster rows keeps them all."""
    a = np.asarray(assign.cpu() if torch.is_tensor(assign) else assign).astype(np.int64)
    if mode not in ("random", "nearest"):
        raise ValueError("select_members: mode is 'random' or 'nearest'")
    if mode == "nearest":
        if best is None:
            raise ValueError("select_members: mode 'nearest' needs best")
        b = np.asarray(best.cpu() if torch.is_tensor(best) else best).astype(np.float64)
    key = _key(seed)
    out = []
    for k in range(K):
        m = [int(i) for i in np.flatnonzero(a == k)]
        take = min(int(per_cluster), len(m))
        if mode == "nearest":
            m.sort(key=lambda i: (-b[i], i))
        else:
            for j in range(take):
                w = philox4x32_10((j, 0, k, 2), key)[0]
                r = j + ((w * (len(m) - j)) >> 32)
                m[j], m[r] = m[r], m[j]
        out.append(m[:take])
    return out


# ------------------------------------------------------------------------------------------------------------------ features
def load_source(path: str, img_dir: str, device):
    """``datasets.SourceDataset`` over a source annotation: the joblib layout of the sample file, or an ``.npz`` with the same keys."""
    from . import datasets as D
    if str(path).endswith(".npz"):
        import joblib
        import tempfile
        with np.load(path, allow_pickle=True) as z:
            d = {k: z[k] for k in z.files}
        with tempfile.TemporaryDirectory() as tmp:
            f = os.path.join(tmp, "source.pt")
            joblib.dump(d, f)
            return D.SourceDataset(f, img_dir=img_dir, device=device)
    return D.SourceDataset(path, img_dir=img_dir, device=device)


def extract_features(model, dataset, batch: int = 32, device=None, workers: int = 8) -> torch.Tensor:
    """``features[5]`` of every row of a ``datasets.SourceDataset`` -> [N][2048] fp32 on `device`: crops cut by the batched
    ``datasets.preprocess_frames`` (what ``ExemplarBank.from_dataset`` does, bit-identical to the single-crop entry), the forward
    ``model(img[lo:hi], need_feature=True)[3][5]`` in slices of `batch` rows, under no_grad with the model in eval mode."""
    from concurrent.futures import ThreadPoolExecutor
    from . import datasets as D
    dev = torch.device(device) if device is not None else dataset.device
    N = len(dataset)
    out = torch.empty(N, FEAT, dtype=torch.float32, device=dev)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad(), ThreadPoolExecutor(max_workers=max(1, workers)) as pool:
            for lo in range(0, N, batch):
                hi = min(N, lo + batch)
                img = torch.empty(hi - lo, 3, 224, 224, dtype=torch.float32, device=dev)
                for a in range(lo, hi, D.CROP_MANY_MAX):
                    b = min(hi, a + D.CROP_MANY_MAX)
                    frames = list(pool.map(lambda i: D.read_image(os.path.join(dataset.img_dir, str(dataset.imgname[i]))), range(a, b)))
                    D.preprocess_frames([torch.from_numpy(f).to(dev) for f in frames],
                                        [np.array(dataset.center[i], dtype=np.float64) for i in range(a, b)],
                                        [float(dataset.scale[i]) for i in range(a, b)], out=img[a - lo:b - lo])
                out[lo:hi] = model(img, need_feature=True)[3][5]
    finally:
        model.train(was_training)
    return out


def load_model(model_file: str, mean_params: str, device):
    """The HMR of a checkpoint ({'model': state_dict}, with or without the MAML wrapper's 'module.' prefix), in eval mode."""
    from .hmr import hmr
    ck = torch.load(model_file, map_location="cpu")["model"]
    model = hmr(mean_params, seed=0).to(device)
    model.load_state_dict({k.replace("module.", ""): v for k, v in ck.items()}, strict=True)
    return model.eval()


# ------------------------------------------------------------------------------------------------------------------ the files
def build_index(source: str, img_dir: str, model_file: str, out: str, clusters: int = 10, per_cluster: int = 10, seed: int = 22,
                select: str = "random", batch: int = 32, n_init: int = 1, features: Optional[str] = None,
                mean_params: str = "data/smpl_mean_params.npz", device="cuda", max_iter: int = 100) -> dict:
    """Write the three retrieval files into `out` and return what went into them.  The sample file is the source annotation
    restricted to the kept rows (cluster after cluster, in draw order), 'index' lists positions in that file, the features file is a
    list of one [n_k][2048] array per cluster whose concatenation is the kept rows' features.  `features`: a ``.npy`` of the full
    [N][2048] matrix - loaded if it exists (no forward passes), written otherwise."""
    import joblib
    dev = torch.device(device)
    ds = load_source(source, img_dir, dev)
    N = len(ds)
    if features and os.path.exists(features):
        feats = torch.from_numpy(np.ascontiguousarray(np.load(features), dtype=np.float32)).to(dev)
        if tuple(feats.shape) != (N, FEAT):
            raise ValueError(f"{features}: expected a [{N}][{FEAT}] matrix")
    else:
        feats = extract_features(load_model(model_file, mean_params, dev), ds, batch=batch, device=dev)
        if features:
            np.save(features, feats.cpu().numpy())
    centers, assign, info = kmeans(feats, clusters, seed, max_iter=max_iter, n_init=n_init)
    picks = select_members(assign, clusters, per_cluster, seed, best=info["best"], mode=select)
    empty = [k for k, m in enumerate(picks) if not m]
    if empty:
        raise RuntimeError(f"retrieval_index: cluster(s) {empty[:8]} are empty (fewer distinct rows than clusters?)")
    kept = [i for m in picks for i in m]
    index, at = [], 0
    for m in picks:
        index.append(list(range(at, at + len(m))))
        at += len(m)
    sample = {}
    for k, v in ds.data.items():
        v = np.asarray(v)
        sample[k] = v[kept] if v.ndim >= 1 and v.shape[0] == N else v
    fh = feats.cpu().numpy()
    feat_list = [fh[m] for m in picks]
    os.makedirs(out, exist_ok=True)
    joblib.dump(sample, os.path.join(out, SAMPLE_FILE))
    joblib.dump(dict(centers=centers.cpu().numpy(), index=index), os.path.join(out, CLUSTER_FILE))
    joblib.dump(feat_list, os.path.join(out, FEATS_FILE))
    return dict(kept=kept, index=index, centers=centers, assign=assign, info=info, features=feats)


def main(argv: Optional[Sequence[str]] = None) -> int:
    p = argparse.ArgumentParser(prog="python -m dynaboa_amd.retrieval_index", description=__doc__.split("\n\n")[0])
    p.add_argument("--source", required=True, help="source annotation: joblib or .npz with keys " + ", ".join(SOURCE_KEYS))
    p.add_argument("--img_dir", required=True)
    p.add_argument("--model_file", required=True)
    p.add_argument("--out", required=True, help="directory for the three files (data/retrieval_res)")
    p.add_argument("--clusters", type=int, default=10)
    p.add_argument("--per_cluster", type=int, default=10)
    p.add_argument("--seed", type=int, default=22)
    p.add_argument("--select", choices=("random", "nearest"), default="random")
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--n_init", type=int, default=1)
    p.add_argument("--features", default=None, help=".npy of the full [N][2048] matrix: loaded if present, written otherwise")
    p.add_argument("--mean_params", default="data/smpl_mean_params.npz")
    p.add_argument("--device", default="cuda")
    o = p.parse_args(argv)
    res = build_index(o.source, o.img_dir, o.model_file, o.out, o.clusters, o.per_cluster, o.seed, o.select, o.batch, o.n_init,
                      o.features, o.mean_params, o.device)
    info = res["info"]
    print(f"retrieval index: {len(res['kept'])} exemplars in {o.clusters} clusters, {info['iterations']} iterations, "
          f"{info['reseeds']} reseeds, objective {info['objective'][-1]:.6f} -> {o.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
