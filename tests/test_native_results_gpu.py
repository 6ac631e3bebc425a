"""--native_results 1 on cuda:0: overlays (--save_res) and prediction dumps (--dump_predictions) stay on the native frame stepper and
work for replica groups and the sharded driver.  The stepper packs every final inference of a frame into its result ring
(csrc/adapt_step.hip); the adaptor writes from there what the autograd path leaves behind.  Everything compared here is equal bit for
bit: ring rows against the stepper's own outputs and against the same sequence adapted alone, files against the autograd path's."""
import os

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

FRAME_ONLY = dict(retrieval=0, lower_level_mixtrain=0, upper_level_mixtrain=0, use_meanteacher=0, use_motion=0,
                  dynamic_boa=0, use_temporal_losses_upper=0, inner_step=1)
FULL = dict(inner_step=1, interval=2, optim_steps=2)
KEYS = ("vts", "rotmat", "shape", "cam")


def _mk(r, opts, expdir=None):
    from dynaboa_amd import benchmark as DB
    from dynaboa_amd.base_adaptor import synthetic_bundle
    o = DB.parser.parse_args([])
    for k, v in opts.items():
        setattr(o, k, v)
    if expdir is not None:
        o.expdir, o.expname = str(expdir), "nr"
    return DB.Adaptor(o, synthetic_bundle(seed=22 + r, identity_pose=False, randomize_norm=True, smpl_seed=0), device="cuda:0")


def _frames(S, NF):
    from dynaboa_amd import assets
    return [[{k: v.to("cuda:0") for k, v in assets.make_frame(100 * r + s, 1, seed=22).items()} for s in range(NF)] for r in range(S)]


def _rows(ns, nframes, r=0):
    """Clones of replica r's ring rows of frames 0 .. nframes - 1 (the ring must hold them all)."""
    assert ns.result_capacity >= nframes
    return [{k: v.clone() for k, v in ns.result(f, r).items()} for f in range(nframes)]


def _same_rows(a, b):
    return all(torch.equal(a[k], b[k]) for k in KEYS)


def _row_equals_outputs(ns, f, r=0):
    row = ns.result(f, r)
    rot, state, vts = ns.output(0, r), ns.output(1, r), ns.output(2, r)
    return (torch.equal(row["rotmat"].reshape(rot.shape), rot) and torch.equal(row["shape"], state[:, 144:154])
            and torch.equal(row["cam"], state[:, 154:157]) and torch.equal(row["vts"], vts))


def _run(ad, frames, after=None):
    ad.reset_records(len(frames))
    out = []
    for step, batch in enumerate(frames):
        ad.global_step = step
        ad.fit_losses = {}
        ad.model.eval()
        out.append(ad.adaptation(batch))
        if after is not None:
            after(step)
    torch.cuda.synchronize()
    return out


def _adam(ad):
    st = ad.optimizer.state[ad.model.module.theta]
    return ad.model.module.theta.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()


def _files(root):
    import joblib
    pics = {n: open(os.path.join(root, "nr", "image", n), "rb").read() for n in sorted(os.listdir(os.path.join(root, "nr", "image")))}
    dumps = {n: joblib.load(os.path.join(root, "nr", "result", n)) for n in sorted(os.listdir(os.path.join(root, "nr", "result")))}
    return pics, dumps


def _same_files(a, b):
    (pa, da), (pb, db) = a, b
    assert sorted(pa) == sorted(pb) == ["Pred_0.png", "Pred_1.png"] and sorted(da) == sorted(db) == ["Pred_0.pt", "Pred_1.pt"]
    for n in pa:
        assert pa[n] == pb[n], n
    for n in da:
        assert sorted(da[n]) == ["beta", "cam", "rotmat", "verts"]
        for k in da[n]:
            assert da[n][k].dtype == db[n][k].dtype and da[n][k].shape == db[n][k].shape and np.array_equal(da[n][k], db[n][k]), (n, k)


# ---------------------------------------------------------------------------- coverage (no GPU needed)
def test_coverage_with_native_results():
    from dynaboa_amd import benchmark as DB, native_step as NS
    assert DB.parser.parse_args([]).native_results == 0
    o = DB.frame_only_options()
    full = DB.parser.parse_args([])
    for flag in ("save_res", "dump_predictions"):
        for opts, want in ((o, "frame"), (full, "full")):
            assert NS.coverage(opts) == (want, None)
            setattr(opts, flag, 1)
            assert NS.coverage(opts) == ("", "rendered results" if flag == "save_res" else "prediction dumps")      # the old answers
            opts.native_results = 1
            assert NS.coverage(opts) == (want, None)
            opts.native_results = 0
            setattr(opts, flag, 0)
    o.native_results, o.save_res, o.second_order = 1, 1, 1
    assert NS.coverage(o) == ("", "second order")                    # everything else in the function is unchanged


# ---------------------------------------------------------------------------- one sequence
@pytest.fixture(scope="module")
def autograd_files(tmp_path_factory):
    """Two frames on the autograd path (what tests/test_save_res_gpu.py pins) with both result flags on, and the native path with every
    result flag off: the files and the state the native results must reproduce."""
    frames = _frames(1, 2)[0]
    root = tmp_path_factory.mktemp("autograd")
    ad = _mk(0, dict(FRAME_ONLY, deferred_metrics=0, save_res=1, dump_predictions=1), root)
    _run(ad, frames)
    assert ad._native is None
    plain = _mk(0, dict(FRAME_ONLY, deferred_metrics=0))
    _run(plain, frames)
    assert plain._native is not None and plain._native.results is None
    return dict(frames=frames, files=_files(root), state=_adam(plain))


@gpu
def test_one_sequence_writes_the_autograd_paths_files_from_the_ring(tmp_path, autograd_files):
    ad = _mk(0, dict(FRAME_ONLY, deferred_metrics=0, save_res=1, dump_predictions=1, native_results=1), tmp_path)
    seen = []
    _run(ad, autograd_files["frames"], after=lambda f: seen.append(_row_equals_outputs(ad._native, f)))
    assert ad._native is not None and ad._native.results is not None and not ad._native.use_side
    assert seen == [True, True]
    _same_files(_files(tmp_path), autograd_files["files"])
    for a, b in zip(_adam(ad), autograd_files["state"]):
        assert torch.equal(a, b)


@gpu
def test_one_sequence_with_the_side_stream_tail(tmp_path, autograd_files):
    """deferred_metrics + overlap_metrics: the frame's final inference is owed to the side stream and issued by the next call or by
    join() - the adaptor joins before it reads the row."""
    ad = _mk(0, dict(FRAME_ONLY, deferred_metrics=1, overlap_metrics=1, save_res=1, dump_predictions=1, native_results=1), tmp_path)
    seen = []

    def after(f):
        ad._native.join()
        seen.append(_row_equals_outputs(ad._native, f))
    _run(ad, autograd_files["frames"], after=after)
    assert ad._native is not None and ad._native.use_side == 1
    assert seen == [True, True]
    _same_files(_files(tmp_path), autograd_files["files"])
    for a, b in zip(_adam(ad), autograd_files["state"]):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------- replica groups
@gpu
def test_full_term_group_rows_equal_the_sequences_alone(tmp_path):
    """Default term set, three sequences, the threshold chosen as tests/test_replica_full_gpu.py chooses it: the sequences leave the
    dynamic loop after different step counts, so their last final inferences live in different activation arenas - every replica's
    row of every frame equals the row the sequence writes alone (default, bit-exact replica policy)."""
    from dynaboa_amd import native_step as NS
    S, NF = 3, 2
    frames = _frames(S, NF)
    gaps = []
    for r in range(S):
        ad = _mk(r, dict(FULL, cos_sim_threshold=-1.0, deferred_metrics=1))
        ad.excute(frames[r][:1], nframes=1)
        gaps.append(1.0 - float(ad.feat_sims[0][0][12]["cos"]))
    thr = float(np.sort(gaps)[S // 2] * 0.999)
    opts = dict(FULL, cos_sim_threshold=thr, deferred_metrics=1, dump_predictions=1, native_results=1)
    alone, steps = [], []
    for r in range(S):
        ad = _mk(r, opts, tmp_path / f"alone{r}")
        ad.excute(frames[r], nframes=NF)
        assert ad._native is not None and ad._native.full
        alone.append(_rows(ad._native, NF))
        steps.append(list(ad.optim_step_record))
    assert len({tuple(s) for s in steps}) > 1, steps                  # the sequences really took different paths
    ads = [_mk(r, opts, tmp_path / "group") for r in range(S)]
    grp = NS.ReplicaGroup(ads, NF)
    assert grp.stepper.full and grp.stepper.S == S
    for s in range(NF):
        grp.step([frames[r][s] for r in range(S)], s, result_steps=[10 * r + s for r in range(S)])
    torch.cuda.synchronize()
    for r in range(S):
        assert list(ads[r].optim_step_record) == steps[r], r
        for f, row in enumerate(_rows(grp.stepper, NF, r)):
            assert _same_rows(row, alone[r][f]), (r, f)
    assert sorted(os.listdir(tmp_path / "group" / "nr" / "result")) == sorted(f"Pred_{10 * r + s}.pt" for r in range(S) for s in range(NF))


@gpu
def test_ended_sequences_rows_are_left_alone(tmp_path, monkeypatch):
    """Lengths 3, 2, 1 (the set-up of test_ragged_sequences_leave_the_active_set), a ring of four rows pre-filled with NaN: a sequence
    that has ended is not written any more - its rows of later frames keep the NaN, its last real row is the alone run's."""
    from dynaboa_amd import benchmark as DB, native_step as NS
    monkeypatch.setattr(NS, "RESULT_RING_ROWS", 4)                    # a row per frame of this test
    lens = [3, 2, 1]
    S = len(lens)
    frames = _frames(S, max(lens))
    fo = dict(vars(DB.frame_only_options(inner_step=3)), deferred_metrics=1, dump_predictions=1, native_results=1)
    alone = []
    for r in range(S):
        ad = _mk(r, fo, tmp_path / f"alone{r}")
        ad.excute(frames[r][:lens[r]], nframes=lens[r])
        alone.append(_rows(ad._native, lens[r]))
    ads = [_mk(r, fo, tmp_path / f"group{r}") for r in range(S)]
    grp = NS.ReplicaGroup(ads, max(lens))
    grp.stepper.results.fill_(float("nan"))
    for s in range(max(lens)):
        grp.step([frames[r][s] if s < lens[r] else None for r in range(S)], s)
    torch.cuda.synchronize()
    for r in range(S):
        for f in range(4):
            row = grp.stepper.results[r, f]
            if f < lens[r]:
                assert _same_rows({k: v for k, v in grp.stepper.result(f, r).items()}, alone[r][f]), (r, f)
            else:
                assert bool(torch.isnan(row).all()), (r, f)
        assert sorted(os.listdir(tmp_path / f"group{r}" / "nr" / "result")) == [f"Pred_{s}.pt" for s in range(lens[r])]


@gpu
def test_throughput_schedule_rows_equal_the_steppers_outputs(tmp_path):
    """Frame-loss set, eight sequences with the replica-aware policy (rep_split = 1: the throughput schedule), one frame."""
    from dynaboa_amd import _lib, benchmark as DB, native_step as NS
    S = 8
    frames = _frames(S, 1)
    fo = dict(vars(DB.frame_only_options(inner_step=1)), deferred_metrics=1, dump_predictions=1, native_results=1)
    import ctypes
    lib = _lib.load()
    saved = {}
    for k in (b"rep_split", b"tp_min"):
        v = ctypes.c_int(0)
        assert lib.dyb_get_option(k, ctypes.byref(v)) == 0
        saved[k] = v.value
    NS.set_replica_policy(True)                                       # rep_split = 1 and tp_min = NS.TP_MIN_SEQUENCES, set explicitly
    try:
        v = ctypes.c_int(0)
        assert lib.dyb_get_option(b"tp_min", ctypes.byref(v)) == 0 and v.value == NS.TP_MIN_SEQUENCES <= S      # S sequences take the throughput schedule
        ads = [_mk(r, fo, tmp_path / f"g{r}") for r in range(S)]
        grp = NS.ReplicaGroup(ads, 1)
        grp.step([frames[r][0] for r in range(S)], 0)
        torch.cuda.synchronize()
    finally:
        for k, val in saved.items():
            lib.dyb_set_option(k, val)
    for r in range(S):
        assert _row_equals_outputs(grp.stepper, 0, r), r
    assert not torch.equal(grp.stepper.result(0, 0)["vts"], grp.stepper.result(0, 1)["vts"])


@gpu
def test_ring_outside_the_logs_block_and_empty_ring_are_refused(tmp_path):
    """A launch scope holds at most 8 per-replica arenas: with replicas the ring must lie inside the one logs block.  Both refusals come
    before any launch - the rings keep their sentinel and the weights stay where they were."""
    from dynaboa_amd import benchmark as DB, native_step as NS
    from dynaboa_amd._abi import check
    S = 3
    frames = _frames(S, 1)
    fo = dict(vars(DB.frame_only_options(inner_step=1)), deferred_metrics=1, dump_predictions=1, native_results=1)
    ads = [_mk(r, fo, tmp_path / f"g{r}") for r in range(S)]
    grp = NS.ReplicaGroup(ads, 1)
    ns = grp.stepper
    outside = torch.full((S, ns.result_capacity, ns.result_floats), -5.0, device="cuda:0")
    ns.results.fill_(-5.0)
    theta = ns.theta.clone()
    check(ns.lib.dyb_stepper_set_p(ns.h, b"results", outside.data_ptr()), "set_p results")
    with pytest.raises(RuntimeError, match="unsupported"):
        ns.adapt_frames([frames[r][0] for r in range(S)])
    check(ns.lib.dyb_stepper_set_p(ns.h, b"results", ns.results.data_ptr()), "set_p results")
    check(ns.lib.dyb_stepper_set_i(ns.h, b"result_capacity", 0), "set_i result_capacity")
    with pytest.raises(RuntimeError, match="bad argument"):
        ns.adapt_frames([frames[r][0] for r in range(S)])
    torch.cuda.synchronize()
    assert bool((outside == -5.0).all()) and bool((ns.results == -5.0).all()) and torch.equal(ns.theta, theta)
    one = _mk(0, fo, tmp_path / "one")
    one.reset_records(1)
    n1 = NS.NativeStepper(one, 1)
    n1.results.fill_(-5.0)
    check(n1.lib.dyb_stepper_set_i(n1.h, b"result_capacity", 0), "set_i result_capacity")
    with pytest.raises(RuntimeError, match="bad argument"):
        n1.adapt_frame(frames[0][0])
    torch.cuda.synchronize()
    assert bool((n1.results == -5.0).all())


# ---------------------------------------------------------------------------- the sharded driver
@gpu
def test_sharded_driver_numbers_overlays_by_global_frame(tmp_path):
    """run_sharded over the five sequences of test_sharded_driver_on_one_gpu_matches_sequences_alone (3, 1, 2, 2, 1 frames), two
    shards, two sequences per GPU, all adaptors writing into ONE exppath: exactly Pred_0.png .. Pred_8.png, each the picture of the
    sequence adapted alone, and the metrics are those of the sequences alone."""
    from dynaboa_amd import benchmark as DB
    from dynaboa_amd.sharded import SequenceSpec, run_sharded
    lens = [3, 1, 2, 2, 1]
    frames = _frames(len(lens), max(lens))
    fo = dict(vars(DB.frame_only_options(inner_step=3)), deferred_metrics=1, save_res=1, native_results=1)
    specs, first = [], 0
    for k, n in enumerate(lens):
        specs.append(SequenceSpec(f"s{k}", first, n, (lambda k=k, n=n: frames[k][:n])))
        first += n
    alone_m, alone_pics = [], []
    for k, n in enumerate(lens):
        ad = _mk(0, fo, tmp_path / f"alone{k}")                      # every sequence starts from the same checkpoint
        res = ad.excute(frames[k][:n], nframes=n)
        assert ad._native is not None
        alone_m += [float(np.ravel(x)[0]) for x in res["mpjpe"]]
        alone_pics += [open(tmp_path / f"alone{k}" / "nr" / "image" / f"Pred_{s}.png", "rb").read() for s in range(n)]
    got = {}
    for rank in (0, 1):
        res = run_sharded(DB.frame_only_options(inner_step=3), specs, lambda: _mk(0, fo, tmp_path / "all"), num_shards=2, shard_rank=rank,
                          seqs_per_gpu=2)
        for gi, m in zip(res["global_index"], res["mpjpe"]):
            assert int(gi) not in got
            got[int(gi)] = float(m)
    assert sorted(got) == list(range(sum(lens)))
    np.testing.assert_allclose([got[i] for i in range(sum(lens))], alone_m, rtol=2e-5)
    names = sorted(os.listdir(tmp_path / "all" / "nr" / "image"), key=lambda n: int(n[5:-4]))
    assert names == [f"Pred_{i}.png" for i in range(sum(lens))]
    for i, n in enumerate(names):
        assert open(tmp_path / "all" / "nr" / "image" / n, "rb").read() == alone_pics[i], n
    assert len(set(alone_pics)) == len(alone_pics)


# ---------------------------------------------------------------------------- overlays over the original frame files
@gpu
def test_group_overlays_over_original_frames_of_two_sizes(tmp_path):
    """Two replicas whose frames are files of different sizes (256 x 128 and 72 x 144, written as
    test_save_results_over_the_original_frames writes them): the group draws both in one ragged launch, and each file equals the
    uniform rendering of that replica's ring row at the frame's own size with the camera converted by its box."""
    from PIL import Image
    from dynaboa_amd import benchmark as DB, native_step as NS
    from dynaboa_amd.render import Renderer, convert_crop_cam_to_orig_img
    rng = np.random.default_rng(4)
    pics = [rng.integers(0, 256, (128, 256, 3), dtype=np.uint8), rng.integers(0, 256, (144, 72, 3), dtype=np.uint8)]
    names = ["seq_a/image_00007.png", "seq_b/image_00001.png"]
    boxes = [[152.0, 52.0, 128.0], [40.5, 81.0, 36.0]]
    for n, f in zip(names, pics):
        os.makedirs(os.path.dirname(tmp_path / "frames" / n), exist_ok=True)
        Image.fromarray(f).save(tmp_path / "frames" / n)
    fo = dict(vars(DB.frame_only_options(inner_step=1)), deferred_metrics=1, save_res=1, native_results=1)
    ads = [_mk(r, fo, tmp_path / "exp") for r in range(2)]
    for a in ads:
        a.imgdir = str(tmp_path / "frames")
    frames = _frames(2, 1)
    batches = []
    for r in range(2):
        b = dict(frames[r][0])
        b["imgname"], b["bbox"] = [names[r]], torch.tensor([boxes[r]], dtype=torch.float64, device="cuda:0")
        batches.append(b)
    grp = NS.ReplicaGroup(ads, 1)
    grp.step(batches, 0, result_steps=[3, 8])
    assert sorted(os.listdir(tmp_path / "exp" / "nr" / "image")) == ["Pred_3.png", "Pred_8.png"]
    for r, n in enumerate((3, 8)):
        row = grp.stepper.result(0, r)
        H, W = pics[r].shape[:2]
        ocam = convert_crop_cam_to_orig_img(row["cam"].float(), torch.tensor([boxes[r]], device="cuda:0"), W, H)
        want = Renderer(resolution=(W, H), faces=ads[r].smpl_neutral.faces).render(
            torch.from_numpy(pics[r]).to("cuda:0"), row["vts"][0].contiguous(), ocam[0], color=ads[r].RESULT_COLOR).cpu().numpy()
        got = np.array(Image.open(tmp_path / "exp" / "nr" / "image" / f"Pred_{n}.png"))
        assert got.shape == pics[r].shape and np.array_equal(got, want), r
