"""--exemplar_bank 1: the device-resident retrieval set (dynaboa_amd/exemplar_bank.py, csrc/retrieval.hip) behind BaseAdaptor.retrieval,
the native stepper and the drivers, on a reference-style data tree (test_asset_formats.data_tree + test_preprocess.populate_stream).
CPU variants run on the kernel emulator; GPU variants are marked gpu.  What decides a pick is checked against the independent fp64 /
Philox check of tests/retrieval_cases.py."""
import numpy as np
import pytest
import torch

import retrieval_cases as RC
from test_asset_formats import data_tree, emu_lib  # noqa: F401  (fixtures)

NOISE = (0.30, 0.45, 0.60)     # |perturbation| / |feature| of the three rewritten centres (see _tree)


def _options(tree, **over):
    from dynaboa_amd import benchmark as DB
    o = DB.parser.parse_args([])
    o.model_file, o.pw3d_root, o.h36m_root = "data/basemodel.pt", tree["imgroot"], tree["h36root"]
    o.expdir = str(tree["root"] / "exps")
    o.interval, o.deferred_metrics = 2, 1
    for k, v in over.items():
        setattr(o, k, v)
    return o


def _tree(data_tree, device, monkeypatch, rewrite_centres=False):
    """The populated tree (once per module).  rewrite_centres: the cluster file's three random centres are replaced - before any bank
    is built from it - by centres NEAR the checkpoint's pooled feature of stream frames 0, 4, 6 (the first frames of the three
    sequences, which hold 4, 2 and 3 frames in stream order): c_k = f_k + e_k with |e_k| = NOISE[k] |f_k|.  A random centre has cosine ~ N(0, 1 / 2048) to every feature, three of
    them can come arbitrarily close; these are separated by their construction (cos(f, f + e) = 1 / sqrt(1 + NOISE^2) = 0.958, 0.912,
    0.857 for equal features) - and every test that relies on it asserts the fp64 margin."""
    import joblib
    from test_preprocess import populate_stream
    from dynaboa_amd import benchmark as DB, exemplar_bank as EB
    monkeypatch.chdir(data_tree["root"])
    if "stream" not in data_tree:
        data_tree["stream"] = populate_stream(data_tree["root"])
        EB._CACHE.clear()
    tree = data_tree["stream"]
    if rewrite_centres and "centres" not in data_tree:
        ad = DB.Adaptor(_options(tree), None, device=device)
        rng = np.random.default_rng(3)
        cs = []
        for k, i in enumerate((0, 4, 6)):
            with torch.no_grad():
                f = ad.model(ad.dataloader.ds[i]["image"].unsqueeze(0), need_feature=True)[3][5][0].double().cpu().numpy()
            e = rng.normal(0, 1, 2048)
            cs.append(f + e * (NOISE[k] * np.linalg.norm(f) / np.linalg.norm(e)))
        path = tree["root"] / "data" / "retrieval_res" / "cluster_res_random_sample_center_10_10_potocol2.pt"
        res = joblib.load(path)
        res["centers"] = np.stack(cs).astype(np.float32)
        joblib.dump(res, path)
        data_tree["centres"] = res
        EB._CACHE.clear()
    return tree


def _cluster(tree):
    import joblib
    res = joblib.load(tree["root"] / "data" / "retrieval_res" / "cluster_res_random_sample_center_10_10_potocol2.pt")
    c = np.asarray(res["centers"], np.float32)
    return c, (1.0 / np.sqrt((c.astype(np.float64) ** 2).sum(1))).astype(np.float32), [list(m) for m in res["index"]]


# ---------------------------------------------------------------------------- 3. bank contents and BaseAdaptor.retrieval
def _bank_contents(device, data_tree, monkeypatch):
    import random
    from dynaboa_amd import benchmark as DB, datasets as D, exemplar_bank as EB
    from dynaboa_amd.base_adaptor import BaseAdaptor
    tree = _tree(data_tree, device, monkeypatch)
    rr = tree["root"] / "data" / "retrieval_res"
    args = (str(rr / "h36m_random_sample_center_10_10.pt"), str(rr / "cluster_res_random_sample_center_10_10_potocol2.pt"), tree["h36root"])
    bank = EB.ExemplarBank.from_tree(*args, device)
    assert EB.ExemplarBank.from_tree(*args, device) is bank                      # one bank per (files, device)
    ds = D.SourceDataset(args[0], img_dir=tree["h36root"], device=device)
    assert bank.items == len(ds) == 12 and bank.clusters == 3 and bank.members == 12
    assert bank.nbytes() >= 12 * 602112
    for i in range(len(ds)):
        it = ds[i]
        for k in EB.KEYS:
            assert getattr(bank, k)[i].cpu().numpy().tobytes() == it[k][0].cpu().numpy().tobytes(), (k, i)
        assert bank.imgname[i] == it["imgname"]
    # BaseAdaptor.retrieval under exemplar_bank = 1 (only the pieces it touches are set up, as in test_preprocess): the items the
    # independent check predicts, draw after draw
    centers, inv, index = _cluster(tree)
    a = BaseAdaptor.__new__(BaseAdaptor)
    a.options = DB.parser.parse_args([])
    a.options.exemplar_bank, a.options.seed = 1, 22
    a.device, a.bundle, a.global_step = torch.device(device), None, 0
    a.load_h36_cluster_res()
    a.h36m_dataset, a.exemplar_bank, a._bank_draw, a._bank_last_pick = ds, bank, 0, None
    rng = np.random.default_rng(8)
    state = random.getstate()
    for draw, k in enumerate((1, 1, 0, 2, 1, 2, 0)):
        x = RC.make_rows(centers, [k], rng)[0]
        c, item, margin = RC.expected_pick(x, centers, inv, index, draw, 22)
        assert c == k and margin >= RC.MARGIN
        got = a.retrieval(torch.from_numpy(x).to(device)[None])
        assert a._bank_last_pick == (c, item) and a._bank_draw == draw + 1
        assert set(got) == {"keypoints", "img", "pose", "betas", "imgname", "pose_3d"} and got["imgname"] == ds[item]["imgname"]
        for key in EB.KEYS:
            assert got[key].shape[0] == 1 and torch.equal(got[key][0], getattr(bank, key)[item]), key
    assert random.getstate() == state                                             # the bank's rule does not touch the `random` stream
    # exemplar_bank = 0: the reference's random.sample behaviour, untouched
    a.exemplar_bank = None
    a.options.exemplar_bank = 0
    feat = torch.from_numpy(centers[1:2] * 0.7 + 0.01).to(device)
    random.seed(5)
    got = a.retrieval(feat)
    random.seed(5)
    want = random.sample([4, 5, 6, 7], 1)[0]
    assert torch.equal(got["pose"][0], ds[want]["pose"][0]) and torch.equal(got["img"][0], ds[want]["img"][0])


def test_bank_refuses_an_empty_cluster():
    """random.sample of an empty cluster raises in the reference; inside a frame on the device nobody could, so such a cluster file is
    refused when the bank is built"""
    from dynaboa_amd import exemplar_bank as EB
    z = lambda *s: torch.zeros(*s)
    tables = dict(img=z(2, 3, 224, 224), keypoints=z(2, 49, 3), pose=z(2, 72), betas=z(2, 10), pose_3d=z(2, 24, 4))
    with pytest.raises(ValueError, match="no members"):
        EB.ExemplarBank(tables, ["a", "b"], np.ones((3, 2048), np.float32), [[0], [], [1]], "cpu")
    with pytest.raises(ValueError, match="outside the set"):
        EB.ExemplarBank(tables, ["a", "b"], np.ones((2, 2048), np.float32), [[0], [2]], "cpu")
    assert EB.ExemplarBank(tables, ["a", "b"], np.ones((2, 2048), np.float32), [[0], [1]], "cpu").members == 2


def test_bank_contents_and_adaptor_retrieval(emu_lib, data_tree, monkeypatch):
    _bank_contents("cpu", data_tree, monkeypatch)


@pytest.mark.gpu
def test_bank_contents_and_adaptor_retrieval_gpu(data_tree, monkeypatch):
    _bank_contents("cuda:0", data_tree, monkeypatch)


# ---------------------------------------------------------------------------- 4. the stepper, one sequence
def _state(ad):
    st = ad.optimizer.state[ad.model.module.theta]
    ns = ad._native
    return dict(theta=ad.model.module.theta.detach().clone(), m=st["exp_avg"].clone(), v=st["exp_avg_sq"].clone(),
                teacher=ad.teacher.theta.detach().clone(), loss=ns.loss_log[getattr(ad, "_native_replica", 0)].clone(),
                picks=ns.picks(getattr(ad, "_native_replica", 0)).clone(), draws=ad._bank_draw, steps=list(ad.optim_step_record))


def _same(a, b, what):
    for k in ("theta", "m", "v", "teacher", "loss", "picks"):
        assert torch.equal(a[k], b[k]), (what, k)
    assert a["draws"] == b["draws"] and a["steps"] == b["steps"], what


def _run_alone(device, tree, idx, monkeypatch, on_device=1, par=1, spy=None, **over):
    from dynaboa_amd import benchmark as DB
    monkeypatch.setenv("DYB_PAR_PASSES", str(par))
    o = _options(tree, exemplar_bank=1, bank_on_device=on_device, **over)
    ad = DB.Adaptor(o, None, device=device)
    if spy is not None:                                          # every retrieval of the callback route: (feature, draw index, pick)
        orig = ad.retrieval

        def wrapped(feature):
            f, d = feature.detach().double().cpu().numpy().reshape(-1), ad._bank_draw
            out = orig(feature)
            spy.append((f, d, ad._bank_last_pick))
            return out
        ad.retrieval = wrapped
    frames = [_collate(ad.dataloader.ds[i]) for i in idx]
    ad.excute(frames, nframes=len(frames))
    assert ad._native is not None and ad._native.full
    assert (ad._native._cb is None) == bool(on_device)
    return ad, _state(ad)


def _collate(item):
    from dynaboa_amd import datasets as D
    return D.collate([item])


def _stepper_one_sequence(device, data_tree, monkeypatch, nframes):
    tree = _tree(data_tree, device, monkeypatch, rewrite_centres=True)
    centers, inv, index = _cluster(tree)
    idx = list(range(nframes))
    spy = []
    _, host = _run_alone(device, tree, idx, monkeypatch, on_device=0, par=1, spy=spy)
    ad, dev1 = _run_alone(device, tree, idx, monkeypatch, on_device=1, par=1)
    _, dev0 = _run_alone(device, tree, idx, monkeypatch, on_device=1, par=0)
    _same(dev1, host, "device route against the callback route")
    _same(dev1, dev0, "par_passes 1 against 0")
    # every retrieval (so also each frame's last one) against the fp64 argmax over the feature it was made from
    assert len(spy) == dev1["draws"] >= 2 * nframes
    seed = int(ad.options.seed)
    for f, d, pick in spy:
        c, item, margin = RC.expected_pick(f.astype(np.float32), centers, inv, index, d, seed)
        print(f"draw {d}: pick {pick} expected {(c, item)} margin {margin:.4f}")
        assert margin >= RC.MARGIN
        assert pick == (c, item) and tuple(dev1["picks"][d % dev1["picks"].shape[0]].tolist()) == (c, item)
    # `_last_h36m` of the device route: built from the latest logged pick when it is read
    last = spy[-1][2][1]
    assert torch.equal(ad._last_h36m["pose"][0], ad.exemplar_bank.pose[last])


@pytest.mark.slow
def test_stepper_one_sequence_emu(emu_lib, data_tree, monkeypatch):
    _stepper_one_sequence("cpu", data_tree, monkeypatch, 4)


@pytest.mark.gpu
def test_stepper_one_sequence_gpu(data_tree, monkeypatch):
    _stepper_one_sequence("cuda:0", data_tree, monkeypatch, 4)


# ---------------------------------------------------------------------------- 5. a replica group of three
@pytest.mark.gpu
def test_replica_group_of_three_gpu(data_tree, monkeypatch):
    from dynaboa_amd import benchmark as DB, native_step as NS
    device = "cuda:0"
    tree = _tree(data_tree, device, monkeypatch, rewrite_centres=True)
    seqs = [[0, 1, 2], [4, 5], [6, 7, 8]]                          # stream frames of each sequence; the second ends a frame early
    alone = [_run_alone(device, tree, s, monkeypatch)[1] for s in seqs]
    ads = [DB.Adaptor(_options(tree, exemplar_bank=1), None, device=device) for _ in seqs]
    assert ads[1].exemplar_bank is ads[0].exemplar_bank           # the group shares one bank
    grp = NS.ReplicaGroup(ads, 3)
    assert grp.stepper._cb is None and grp.stepper.S == 3
    ds = ads[0].dataloader.ds
    for s in range(3):
        before = ads[1]._bank_draw
        grp.step([_collate(ds[q[s]]) if s < len(q) else None for q in seqs], s)
        if s >= len(seqs[1]):
            assert ads[1]._bank_draw == before                    # the ended sequence draws nothing more
    for r, ad in enumerate(ads):
        got = _state(ad)
        n = len(seqs[r])
        for k in ("theta", "m", "v", "teacher", "picks"):
            assert torch.equal(got[k], alone[r][k]), (r, k)
        assert torch.equal(got["loss"][:n], alone[r]["loss"][:n]), r
        assert got["draws"] == alone[r]["draws"] and got["steps"] == alone[r]["steps"], r


# ---------------------------------------------------------------------------- 6. stream order on the emulator
@pytest.mark.slow
@pytest.mark.parametrize("order", [0, 1], ids=["chain_first", "side_streams_first"])
def test_bank_parallel_passes_under_adversarial_stream_order(emu_lib, data_tree, monkeypatch, order):
    """One full-term frame (a lower and an upper level, each with a labelled term) with the bank on the device and par_passes 1 in the
    emulator's lazy stream mode, drained chain-first or side-stream-first, equals the in-line sequential run (par_passes 0; computed
    once for both orders) bit for bit: feat5 -> select -> gather -> exemplar forward and the reuse of the exemplar staging by the
    second level each have their event."""
    from types import SimpleNamespace
    from dynaboa_amd import _lib, native_step as NS
    raw = _lib.load()
    tree = _tree(data_tree, "cpu", monkeypatch, rewrite_centres=True)
    # (no dynamic-BOA gate: its host poll cannot run inside a lazy section)
    if "sequential_frame" not in data_tree:
        data_tree["sequential_frame"] = _run_alone("cpu", tree, [0], monkeypatch, on_device=1, par=0, dynamic_boa=0)[1]
    orig = NS.NativeStepper.adapt_frame_full
    used = []

    def wrapped(self, *a, **kw):
        self._aux = SimpleNamespace(cuda_stream=1)          # any non-null handle is a second stream to the emulator
        raw.emu_lazy(1)
        try:
            return orig(self, *a, **kw)
        finally:
            used.append(raw.emu_flush(order))
            raw.emu_lazy(0)
    monkeypatch.setattr(NS.NativeStepper, "adapt_frame_full", wrapped)
    _, st = _run_alone("cpu", tree, [0], monkeypatch, on_device=1, par=1, dynamic_boa=0)
    assert used and used[0] >= 3, used                       # chain + auxiliary + exemplar stream
    assert st["draws"] == 2
    _same(data_tree["sequential_frame"], st, "lazy stream order")


# ---------------------------------------------------------------------------- 7. the driver
def _driver(device, data_tree, monkeypatch):
    from dynaboa_amd import benchmark as DB, native_step as NS, sharded
    tree = _tree(data_tree, device, monkeypatch, rewrite_centres=False)
    o = _options(tree, exemplar_bank=1, seqs_per_gpu=2, num_shards=1)
    made = []
    orig = NS.NativeStepper.__init__

    def spy(self, *a, **kw):
        orig(self, *a, **kw)
        made.append(self)
    monkeypatch.setattr(NS.NativeStepper, "__init__", spy)
    ads = []

    def make():
        ads.append(DB.Adaptor(o, None, device=device))
        return ads[-1]
    # the 4- and the 3-frame sequence in lockstep as a group of two, then the 2-frame one alone through excute()
    res = sharded.run_sharded(o, sharded.pw3d_sequences(o, torch.device(device)), make, 1, 0, 2)
    for k in ("mpjpe", "pampjpe", "pve"):
        assert np.isfinite(np.asarray(res[k], np.float64)).all() and len(np.ravel(res[k])) == 9, k
    assert len(made) == 2 and made[0].S == 2 and made[1].S == 1
    assert all(ns._cb is None and ns._bank_dev for ns in made)                # no retrieval callback is registered
    assert len(ads) == 3 and all(a._bank_draw >= 2 for a in ads)
    for a in ads:                                                             # the labelled-loss summaries of each sequence's last frame
        assert {"ll/labled_loss", "ul/labled_loss", "teacher/loss"} <= set(a.fit_losses), sorted(a.fit_losses)
        assert all(np.isfinite(float(a.fit_losses[k])) for k in ("ll/labled_loss", "ul/labled_loss"))


@pytest.mark.gpu
def test_sharded_driver_with_the_bank_gpu(data_tree, monkeypatch):
    _driver("cuda:0", data_tree, monkeypatch)
