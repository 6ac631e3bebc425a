"""dynaboa_amd/retrieval_index.py: the Lloyd loop on designed data against its fp64 restatement (tests/kmeans_cases.py; emulator and,
marked gpu, the device), the documented Philox rules of the initial draw and of select_members against host restatements, and - gpu
only - the feature extraction and the whole builder on a seeded tree of 24 small exemplar images with the synthetic checkpoint.
The procedure is this project's own (the reference ships its index as a download and neither its checkpoint nor Human3.6M is at hand):
what is pinned here are the stated rules, not the authors' files."""
import os

import numpy as np
import pytest
import torch

import kmeans_cases as KC
from test_asset_formats import emu_lib  # noqa: F401  (fixture)


@pytest.fixture(scope="module")
def blobs():
    x, blob = KC.blob_data()
    inits = KC.blob_inits()
    return x, blob, inits, {name: KC.lloyd64(x, init) for name, init in inits.items()}


def _centre_bound(x, assign, K):
    """fp64 means of the unit rows and the bound a fp32 centre must meet: gamma_(n_k + 2) for the mean (kmeans_cases.check_update)
    and, because this reference normalises in fp64 where the kernel takes fp32 inverse norms, their relative rounding gamma_(D + 3)
    (kmeans_cases.check_inv_norm) on top - (1 + a)(1 + b) - 1 of sum |x_ij| / |x_i| / n_k"""
    x64 = x.astype(np.float64)
    xn = x64 / np.sqrt((x64 ** 2).sum(1))[:, None]
    want, bound = np.zeros((K, x.shape[1])), np.zeros((K, x.shape[1]))
    for k in range(K):
        m = assign == k
        n = int(m.sum())
        want[k] = xn[m].sum(0) / n
        bound[k] = ((1 + KC.gamma(n + 2)) * (1 + KC.gamma(x.shape[1] + 3)) - 1) * np.abs(xn[m]).sum(0) / n
    return want, bound


def _lloyd_designed(device, blobs):
    from dynaboa_amd import retrieval_index as RI
    x, _, inits, refs = blobs
    feats = torch.from_numpy(x).to(device)
    for name, init in inits.items():
        ref, trace = refs[name], []
        centers, assign, info = RI.lloyd(RI._torch_ops(feats, KC.BLOBS), init, max_iter=100, trace=trace)
        assert info["iterations"] == ref["iterations"] == len(trace) and info["reseeds"] == ref["reseeds"], name
        for it, (got, want) in enumerate(zip(trace, ref["assign"])):
            assert np.array_equal(got, want), (name, it)
        assert np.array_equal(assign, ref["assign"][-1])
        want, bound = _centre_bound(x, assign, KC.BLOBS)
        assert np.abs(want - ref["centers"]).max() < 1e-12                      # the restated run ends on the means of its assignment
        assert (np.abs(centers.astype(np.float64) - want) <= bound).all(), name
        assert len(info["objective"]) == info["iterations"] and info["best"].shape == (KC.BLOB_N,)
        # the public entry: the same run, tensors on the device
        c2, a2, i2 = RI.kmeans(feats, KC.BLOBS, seed=1, init=torch.from_numpy(init))
        assert c2.device == feats.device and c2.cpu().numpy().tobytes() == centers.tobytes() and np.array_equal(a2.cpu().numpy(), assign)
        assert i2["objective"] == info["objective"]
    # init=None: the documented Philox draw, then the same loop
    for seed in (22, (5 << 32) | 9):
        rows = KC.philox_init_rows(KC.BLOB_N, KC.BLOBS, seed)
        assert RI.init_rows(KC.BLOB_N, KC.BLOBS, seed) == rows and len(set(rows)) == KC.BLOBS
        c, a, i = RI.kmeans(feats, KC.BLOBS, seed=seed)
        ce, ae, ie = RI.kmeans(feats, KC.BLOBS, seed=0, init=x[rows])
        assert c.cpu().numpy().tobytes() == ce.cpu().numpy().tobytes() and torch.equal(a, ae) and i["objective"] == ie["objective"]
    # n_init: seeds seed, seed + 1, ...; the highest final objective wins, the first on a tie
    runs = [RI.kmeans(feats, KC.BLOBS, seed=40 + r) for r in range(3)]
    objs = [r[2]["objective"][-1] for r in runs]
    c, a, i = RI.kmeans(feats, KC.BLOBS, seed=40, n_init=3)
    assert i["seed"] == 40 + int(np.argmax(objs)) and torch.equal(a, runs[int(np.argmax(objs))][1])


def test_lloyd_on_designed_data_emu(emu_lib, blobs):
    _lloyd_designed("cpu", blobs)


@pytest.mark.gpu
def test_lloyd_on_designed_data_gpu(blobs):
    _lloyd_designed("cuda:0", blobs)


def test_init_rows_edges():
    from dynaboa_amd import retrieval_index as RI
    for N, K, seed in ((1, 1, 0), (7, 7, 3), (300000, 100, 22)):
        rows = RI.init_rows(N, K, seed)
        assert rows == KC.philox_init_rows(N, K, seed) and len(set(rows)) == K and all(0 <= r < N for r in rows)
    with pytest.raises(ValueError):
        RI.init_rows(3, 4, 0)


def test_select_members():
    from dynaboa_amd import retrieval_index as RI
    rng = np.random.default_rng(3)
    K = 6
    assign = rng.integers(0, 4, 500)                     # clusters 0 .. 3 large
    assign[:3] = 4                                       # cluster 4: three rows; cluster 5: none
    best = rng.uniform(0.2, 0.9, 500).astype(np.float32)
    best[10], best[20] = best[30], best[30]              # a three-way tie inside a cluster
    assign[[10, 20, 30]] = 2
    best[[10, 20, 30]] = 0.95                            # ... at the top: rows 10, 20, 30 in that order
    members = [set(np.flatnonzero(assign == k).tolist()) for k in range(K)]
    got = RI.select_members(assign, K, 10, seed=22)
    assert got == KC.philox_select(assign, K, 10, 22)
    again = RI.select_members(torch.from_numpy(assign), K, 10, seed=22)
    other = RI.select_members(assign, K, 10, seed=23)
    assert again == got and other != got and all(other[k] != got[k] for k in range(4))
    for picks in (got, other):
        for k in range(K):
            assert len(set(picks[k])) == len(picks[k]) == min(10, len(members[k])) and set(picks[k]) <= members[k]
        assert sorted(picks[4]) == [0, 1, 2] and picks[5] == []
    near = RI.select_members(assign, K, 4, seed=22, best=best, mode="nearest")
    for k in range(K):
        want = sorted(members[k], key=lambda i: (-float(best[i]), i))[:4]
        assert near[k] == want
    assert near[2][:3] == [10, 20, 30]
    with pytest.raises(ValueError):
        RI.select_members(assign, K, 4, seed=1, mode="nearest")


# ------------------------------------------------------------------------------------------------------------------ builder (gpu)
M = 24


def _source_tree(root):
    """24 seeded exemplar images and their annotation, in the manner of test_preprocess.populate_stream's exemplar set, plus the
    synthetic checkpoint and mean parameters as files"""
    import joblib
    from test_preprocess import _write_png
    from dynaboa_amd.base_adaptor import synthetic_bundle
    rng = np.random.default_rng(31)
    names = []
    for i in range(M):
        rel = f"S{1 + i % 3}/img_{i:04d}.png"
        _write_png(str(root / "h36m_images" / rel), rng.integers(0, 256, (72 + 8 * (i % 3), 80, 3), dtype=np.uint8))
        names.append(rel)
    src = dict(imgname=np.array(names), scale=rng.uniform(0.25, 0.4, M), center=rng.uniform(30, 50, (M, 2)), pose=rng.normal(0, 0.2, (M, 72)),
               shape=rng.normal(0, 0.5, (M, 10)), S=np.concatenate([rng.normal(0, 0.3, (M, 24, 3)), np.ones((M, 24, 1))], 2),
               part=np.concatenate([rng.uniform(0, 80, (M, 24, 2)), (rng.random((M, 24, 1)) < 0.8).astype(float)], 2))
    (root / "data").mkdir()
    joblib.dump(src, root / "data" / "source.pt")
    np.savez(root / "data" / "source.npz", **src)
    bundle = synthetic_bundle()
    torch.save(bundle.checkpoint, root / "data" / "basemodel.pt")
    np.savez(root / "data" / "smpl_mean_params.npz", **bundle.mean_params)
    return src


@pytest.mark.gpu
def test_extract_features_and_builder_gpu(tmp_path, monkeypatch):
    import joblib
    from dynaboa_amd import benchmark as DB, datasets as D, exemplar_bank as EB, retrieval_index as RI
    from dynaboa_amd.base_adaptor import BaseAdaptor
    dev = torch.device("cuda:0")
    src = _source_tree(tmp_path)
    monkeypatch.chdir(tmp_path)
    img_dir = str(tmp_path / "h36m_images")
    ds = D.SourceDataset("data/source.pt", img_dir=img_dir, device=dev)
    model = RI.load_model("data/basemodel.pt", "data/smpl_mean_params.npz", dev)
    # extract_features: bit for bit the forward over the same slices of the crops the exemplar bank cuts
    feats = RI.extract_features(model, ds, batch=10, device=dev)
    bank = EB.ExemplarBank.from_dataset(ds, np.ones((1, 2048), np.float32), [list(range(M))], dev)
    assert tuple(feats.shape) == (M, 2048)
    with torch.no_grad():
        for lo in range(0, M, 10):
            want = model(bank.img[lo:lo + 10], need_feature=True)[3][5]
            assert torch.equal(feats[lo:lo + 10], want), lo
    ds_npz = RI.load_source("data/source.npz", img_dir, dev)
    assert len(ds_npz) == M and list(ds_npz.imgname) == list(ds.imgname) and np.array_equal(ds_npz.pose, ds.pose)

    # the command line, twice with the same seed
    def run(out):
        rc = RI.main(["--source", "data/source.pt", "--img_dir", img_dir, "--model_file", "data/basemodel.pt", "--out", out,
                      "--clusters", "3", "--per_cluster", "4", "--batch", "10", "--features", "data/full_feats.npy"])
        assert rc == 0
        return [joblib.load(os.path.join(out, f)) for f in (RI.SAMPLE_FILE, RI.CLUSTER_FILE, RI.FEATS_FILE)]
    sample, cluster, flist = run("data/retrieval_res")
    full = np.load("data/full_feats.npy")
    assert full.tobytes() == feats.cpu().numpy().tobytes()                       # --features wrote the full matrix ...
    sample2, cluster2, flist2 = run("data/second")                               # ... and the second run loads it: no forward passes
    assert set(sample) == set(src) == set(sample2)
    for k in src:
        assert np.array_equal(sample[k], sample2[k]), k
    assert np.asarray(cluster["centers"]).tobytes() == np.asarray(cluster2["centers"]).tobytes() and cluster["index"] == cluster2["index"]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(flist, flist2)) and len(flist) == len(flist2) == 3
    # the three loaders
    kept_ds = D.SourceDataset(os.path.join("data/retrieval_res", RI.SAMPLE_FILE), img_dir=img_dir, device=dev)
    a = BaseAdaptor.__new__(BaseAdaptor)
    a.options = DB.parser.parse_args([])
    a.device, a.bundle = dev, None
    a.load_h36_cluster_res()
    assert tuple(a.centers.shape) == (3, 2048) and a.h36m_cluster_res["index"] == cluster["index"]
    EB._CACHE.clear()
    kept_bank = EB.ExemplarBank.from_tree(os.path.join("data/retrieval_res", RI.SAMPLE_FILE), os.path.join("data/retrieval_res", RI.CLUSTER_FILE),
                                          img_dir, dev)
    EB._CACHE.clear()
    n = len(kept_ds)
    assert kept_bank.items == n == kept_bank.members and kept_bank.clusters == 3
    # no cluster is empty, every kept row is in exactly one member list, at most 4 per cluster
    index = cluster["index"]
    assert all(1 <= len(m) <= 4 for m in index) and sorted(i for m in index for i in m) == list(range(n))
    # sample-file row j carries the annotation of the source row it came from (image names are unique)
    origin = [list(src["imgname"]).index(nm) for nm in sample["imgname"]]
    assert len(set(origin)) == n
    for k in src:
        assert np.array_equal(np.asarray(sample[k]), np.asarray(src[k])[origin]), k
    assert kept_bank.img.cpu().numpy().tobytes() == bank.img[origin].cpu().numpy().tobytes()
    # the features file: per cluster, and its concatenation = the kept rows of the full matrix
    assert [len(f) for f in flist] == [len(m) for m in index]
    assert np.concatenate(flist).tobytes() == full[origin].tobytes()
