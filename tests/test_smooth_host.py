"""Temporal smoothing: the host side.  dynaboa_amd.smooth (weights, the tensor wrappers, the pass over dumps, the 3DPW pass with metrics),
the drivers' flags and the scene functions' new keywords on the emulator library with CPU tensors (the `emu_lib` pattern of
tests/test_seq_metrics_host.py) and the synthetic bundle's SMPL; marked gpu, the internet driver with --smooth_window and the online
adaptor with --one_euro on cuda:0."""
import csv
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import smooth_cases as SM
from conftest import GOLDEN


@pytest.fixture
def emu_lib():
    from emu.build_emu import build
    from dynaboa_amd import _abi, _lib
    lib = _abi.bind(ctypes.CDLL(build()))
    saved = _lib._lib
    _lib.use_library(lib)
    yield lib
    _lib._lib = saved


@pytest.fixture(scope="module")
def bundle():
    from dynaboa_amd.base_adaptor import synthetic_bundle
    return synthetic_bundle(seed=22, identity_pose=False, randomize_norm=True, smpl_seed=0)


def cam_t_of(cam):
    s, tx, ty = (np.float32(c) for c in cam)
    return np.array([[tx, ty, np.float32(2 * 5000.) / (np.float32(224) * s + np.float32(1e-9))]], np.float32)


def write_dumps(folder, rows, x, index):
    """Pred_{n}.pt for `rows`, row n from frame index[n] of the inputs x, in the shapes a batch-size-1 run dumps."""
    import joblib
    os.makedirs(folder, exist_ok=True)
    rng = np.random.default_rng(3)
    for n in rows:
        i = index[n]
        joblib.dump({'verts': rng.normal(0, 1, (1, 6890, 3)).astype(np.float32), 'cam': cam_t_of(x["cam"][i]),
                     'rotmat': x["rotmat"][i].reshape(1, 24, 3, 3).copy(), 'beta': x["betas"][i].reshape(1, 10).copy()},
                    os.path.join(folder, f"Pred_{n}.pt"))


# ------------------------------------------------------------------------------------------------ weights and wrappers
def test_gaussian_weights():
    from dynaboa_amd.smooth import gaussian_weights
    w = gaussian_weights(4)
    assert w.dtype == np.float32 and w.shape == (9,) and w[4] == 1 and np.array_equal(w, w[::-1])
    k = np.arange(-4, 5, dtype=np.float64)
    assert np.array_equal(w, np.exp(-0.5 * (k / 2.0) ** 2).astype(np.float32))             # sigma = half_window / 2, one rounding
    assert np.array_equal(gaussian_weights(3, 1.5), np.exp(-0.5 * (np.arange(-3, 4) / 1.5) ** 2).astype(np.float32))
    assert np.array_equal(gaussian_weights(0), np.ones(1, np.float32))
    for bad in (-1, 33):
        with pytest.raises(ValueError):
            gaussian_weights(bad)
    with pytest.raises(ValueError):
        gaussian_weights(2, 0.0)
    for h in (1, 4, 8, 32):
        assert np.array_equal(gaussian_weights(h), SM.gaussian(h))


def test_smooth_sequences_wrapper(emu_lib):
    """Tensors in, tensors of the same shapes out, against the restatement; lengths that do not tile the frames are refused."""
    from dynaboa_amd.smooth import smooth_sequences
    x = SM.make_inputs()
    n = sum(SM.LENGTHS)
    rot, betas, cam = (torch.from_numpy(x[k]) for k in ("rotmat", "betas", "cam"))
    valid = np.ones(n, bool)
    valid[30] = False
    R, B, C = smooth_sequences(rot.reshape(n, 24, 3, 3), betas, cam, lengths=SM.LENGTHS, valid=torch.from_numpy(valid), half_window=4, sigma=2.0)
    assert R.shape == (n, 24, 3, 3) and B.shape == betas.shape and C.shape == cam.shape
    ref = SM.ref_smooth(x["rotmat"], x["betas"], x["cam"], SM.LENGTHS, SM.gaussian(4, 2.0), 4, valid=valid)
    SM.check((R.reshape(n, 24, 9).numpy(), B.numpy(), C.numpy()), ref)
    R2, B2, C2 = smooth_sequences(rot, lengths=SM.LENGTHS, half_window=2, weights=[1, 2, 3, 2, 1])
    assert R2.shape == rot.shape and B2 is None and C2 is None
    SM.check((R2.numpy(), None, None), SM.ref_smooth(x["rotmat"], None, None, SM.LENGTHS, [1, 2, 3, 2, 1], 2))
    with pytest.raises(ValueError):
        smooth_sequences(rot, lengths=[3, 3])
    with pytest.raises(ValueError):
        smooth_sequences(rot, lengths=SM.LENGTHS, half_window=2, weights=[1, 2, 1])
    with pytest.raises(RuntimeError, match="dyb_smooth_sequences"):
        smooth_sequences(rot, lengths=SM.LENGTHS, half_window=1, weights=[1, 0, 1])
    e = smooth_sequences(rot[:0], betas[:0], lengths=[0])
    assert e[0].shape == (0, 24, 9) and e[1].shape == (0, 10)


def test_one_euro_class(emu_lib):
    """OneEuro.step against the restatement over 6 steps; an inactive sequence returns its input and keeps its state; reset."""
    from dynaboa_amd.smooth import OneEuro
    rot, betas, cam = SM.oe_stream()
    f = OneEuro(SM.OE_R, fps=30.0, min_cutoff=1.0, beta=0.5, d_cutoff=1.0, J=SM.J, nb=SM.NB, nc=SM.NC, device="cpu")
    assert f.state.shape == (SM.OE_R, 1 + 2 * (4 * SM.J + SM.NB + SM.NC)) and not f.state.any()
    state = [dict(started=False, xh=None, dxh=None) for _ in range(SM.OE_R)]
    for t in range(6):
        active = [True, t != 3, True]
        if t == 4:
            f.reset(2)
            state[2] = dict(started=False, xh=None, dxh=None)
        before = f.state.clone()
        R, B, C = f.step(torch.from_numpy(rot[t]).reshape(SM.OE_R, SM.J, 3, 3), torch.from_numpy(betas[t]), torch.from_numpy(cam[t]),
                         active=None if all(active) else active)
        assert R.shape == (SM.OE_R, SM.J, 3, 3)
        ref = SM.ref_one_euro_step(state, rot[t], betas[t], cam[t], np.array(active), **SM.OE)
        on = np.array(active)
        SM.check((R.reshape(SM.OE_R, SM.J, 9).numpy()[on], B.numpy()[on], C.numpy()[on]), [v[on] for v in ref], SM.OE_BOUND)
        if t == 3:
            assert torch.equal(f.state[1], before[1]) and R[1].reshape(-1).numpy().tobytes() == rot[t][1].tobytes()
        if t in (0, 4):
            assert R[2].reshape(-1).numpy().tobytes() == rot[t][2].tobytes() and B[2].numpy().tobytes() == betas[t][2].tobytes()
    f.reset()
    assert not f.state.any()
    with pytest.raises(ValueError):
        OneEuro(1, fps=0.0, device="cpu")


# ------------------------------------------------------------------------------------------------ the pass over dumps
SEQ_ROWS = [[0, 2, 4, 6, 8, 10, 12], [1, 3, 5]]


def _dump_case(tmp_path):
    x = SM.make_inputs((7, 3), seed=41)
    index = {n: i for i, n in enumerate(SEQ_ROWS[0] + SEQ_ROWS[1])}
    index[7] = 0                                                       # a dump no sequence lists
    exp = str(tmp_path / "run")
    write_dumps(os.path.join(exp, "result"), list(index), x, index)
    return exp, x


def test_smooth_results_writes_the_rows_files_with_the_sources_keys(emu_lib, bundle, tmp_path):
    import joblib
    from dynaboa_amd.smooth import smooth_results
    from dynaboa_amd.smpl import SMPL
    smpl = SMPL(tables=bundle.smpl_neutral)
    exp, x = _dump_case(tmp_path)
    camf = np.random.default_rng(5).normal(0, 1, (10, 4)).astype(np.float32)
    paths = smooth_results(exp, SEQ_ROWS, smpl, half_window=2, cam_frame=camf)
    rows = SEQ_ROWS[0] + SEQ_ROWS[1]
    assert paths == [os.path.join(exp, "result_smooth", f"Pred_{n}.pt") for n in rows]
    assert sorted(os.listdir(os.path.join(exp, "result_smooth"))) == sorted(f"Pred_{n}.pt" for n in rows)      # row 7 is in no sequence
    ref = SM.ref_smooth(x["rotmat"], x["betas"], camf, (7, 3), SM.gaussian(2), 2)
    for i, n in enumerate(rows):
        src, out = joblib.load(os.path.join(exp, "result", f"Pred_{n}.pt")), joblib.load(paths[i])
        assert sorted(out) == sorted(list(src) + ["cam_frame"])
        for k in src:
            assert out[k].shape == src[k].shape and out[k].dtype == src[k].dtype, k
        assert out["cam"].tobytes() == src["cam"].tobytes()                                 # the frame's own crop camera, untouched
        SM.check((out["rotmat"].reshape(1, 24, 9), out["beta"], out["cam_frame"].reshape(1, 4)), [r[i:i + 1] for r in ref])
        with torch.no_grad():
            r = torch.from_numpy(out["rotmat"])
            v = smpl(betas=torch.from_numpy(out["beta"]), body_pose=r[:, 1:], global_orient=r[:, 0].unsqueeze(1), pose2rot=False).vertices
        assert np.abs(out["verts"] - v.numpy()).max() <= 1e-5 and not np.array_equal(out["verts"], src["verts"])
    # without cam_frame: exactly the source's keys; frame ids with a gap split the first sequence into 0,2,4 | 6..12
    paths = smooth_results(exp, SEQ_ROWS, smpl, half_window=2, frame_ids=[[0, 1, 2, 10, 11, 12, 13], [5, 6, 7]], dst="other")
    out = joblib.load(paths[2])
    assert sorted(out) == ["beta", "cam", "rotmat", "verts"]
    ref = SM.ref_smooth(x["rotmat"], x["betas"], None, (3, 4, 3), SM.gaussian(2), 2)
    SM.check((out["rotmat"].reshape(1, 24, 9), out["beta"], None), [ref[0][2:3], ref[1][2:3], None])
    # a callable camera sees (row, dump)
    seen = []
    smooth_results(exp, SEQ_ROWS[1:], smpl, half_window=1, cam_frame=lambda n, d: (seen.append((n, sorted(d))), np.ones(4, np.float32))[1], dst="third")
    assert seen == [(n, ["beta", "cam", "rotmat", "verts"]) for n in SEQ_ROWS[1]]
    assert sorted(os.listdir(os.path.join(exp, "third"))) == ["Pred_1.pt", "Pred_3.pt", "Pred_5.pt"]


def test_smooth_results_in_chunks_of_whole_sequences_writes_the_same_bytes(emu_lib, bundle, tmp_path, monkeypatch):
    """A chunk limit below the first sequence's length: one call per sequence, the same files as one call over both."""
    from dynaboa_amd import smooth as S
    from dynaboa_amd.smpl import SMPL
    smpl = SMPL(tables=bundle.smpl_neutral)
    exp, x = _dump_case(tmp_path)
    camf = np.random.default_rng(5).normal(0, 1, (10, 4)).astype(np.float32)
    one = S.smooth_results(exp, SEQ_ROWS, smpl, half_window=2, cam_frame=camf, dst="one")
    calls = []
    inner = S.smooth_sequences
    monkeypatch.setattr(S, "smooth_sequences", lambda *a, **k: (calls.append(k["lengths"]), inner(*a, **k))[1])
    monkeypatch.setattr(S, "SMOOTH_CHUNK", 3)
    two = S.smooth_results(exp, SEQ_ROWS, smpl, half_window=2, cam_frame=camf, dst="two")
    assert calls == [[7], [3]] and [os.path.basename(p) for p in one] == [os.path.basename(p) for p in two]
    assert all(open(a, "rb").read() == open(b, "rb").read() for a, b in zip(one, two))


def test_smooth_results_names_a_missing_file_and_refuses_batches(emu_lib, bundle, tmp_path):
    import joblib
    from dynaboa_amd.smooth import smooth_results
    from dynaboa_amd.smpl import SMPL
    smpl = SMPL(tables=bundle.smpl_neutral)
    exp, x = _dump_case(tmp_path)
    os.remove(os.path.join(exp, "result", "Pred_4.pt"))
    with pytest.raises(FileNotFoundError, match=r"row 4 .*Pred_4\.pt"):
        smooth_results(exp, SEQ_ROWS, smpl, half_window=2)
    d = joblib.load(os.path.join(exp, "result", "Pred_3.pt"))
    joblib.dump({k: np.concatenate([v, v]) for k, v in d.items()}, os.path.join(exp, "result", "Pred_3.pt"))
    with pytest.raises(ValueError, match="batch-size-1"):
        smooth_results(exp, SEQ_ROWS[1:], smpl, half_window=2)


def test_parser_defaults_are_off():
    from dynaboa_amd import benchmark as DB, internet as I, online as ON, smooth as S
    o = I.parser.parse_args([])
    assert o.smooth_window == 0 and o.smooth_sigma is None
    assert not hasattr(DB.parser.parse_args([]), "smooth_window") and not hasattr(DB.parser.parse_args([]), "half_window")
    o = ON.parser.parse_args([])
    assert (o.one_euro, o.one_euro_min_cutoff, o.one_euro_beta, o.fps) == (0, 1.0, 0.0, 30.0)
    assert ON.online_options().one_euro == 0 and ON.make_one_euro(ON.online_options(), 1, "cpu") is None
    o = S._make_parser().parse_args(["--expdir", "d", "--expname", "n"])
    assert (o.half_window, o.sigma, o.expdir, o.expname, o.write_results) == (4, None, "d", "n", 0)


def test_smooth_window_with_shards_is_refused_before_any_adaptation(tmp_path, monkeypatch):
    from dynaboa_amd import internet as I
    monkeypatch.setattr(I, "Adaptor", lambda *a, **k: pytest.fail("an adaptor was built"))
    monkeypatch.setattr(I, "InternetDataset", lambda *a, **k: pytest.fail("the dataset was read"))
    o = I.parser.parse_args(["--internet_root", str(tmp_path), "--expdir", str(tmp_path / "none"), "--expname", "run", "--num_shards", "2",
                             "--smooth_window", "2"])
    with pytest.raises(ValueError, match=r"--compose_only 1"):
        I.run_driver(o, device=torch.device("cpu"))
    assert not os.path.exists(tmp_path / "none")


# ------------------------------------------------------------------------------------------------ the scene functions' keywords
def test_scene_functions_defaults_and_new_keywords(emu_lib, tmp_path):
    """compose_scenes / scene_meshes with default keywords read result/ and write scene/ as before - another folder beside them
    changes nothing; with result_dir / out_dir they read and write there, and a dump's cam_frame is the camera drawn under."""
    import joblib
    from PIL import Image
    from dynaboa_amd import internet as I
    from dynaboa_amd.render import Renderer
    from render_cases import icosphere
    root, exp = tmp_path / "video", str(tmp_path / "exp" / "run")
    os.makedirs(root / "images" / "vid")
    rng = np.random.default_rng(11)
    W, H = 64, 48
    for f in range(2):
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(root / "images" / "vid" / f"{f:06d}.png")
    np.savez(root / "vid.npz", imgname=[f"vid/{f:06d}.png" for f in range(2)], center=[(30.0, 22.0), (30.0, 24.0)], scale=[34.0 / 200] * 2,
             part=np.zeros((2, 49, 3)), track=np.zeros(2, np.int64))
    v, faces = icosphere(1)
    verts = v.astype(np.float32)
    verts[:, 2] += 3.0
    for sub, extra in (("result", {}), ("result_smooth", {"cam_frame": np.array([0.3, 0.4, 0.2, -0.1], np.float32)})):
        os.makedirs(os.path.join(exp, sub))
        for n in range(2):
            joblib.dump({'verts': verts[None] * np.float32(1.0 if sub == "result" else 0.8), 'cam': cam_t_of((0.9, 0.05, -0.1)),
                         'rotmat': np.zeros((1, 24, 3, 3), np.float32), 'beta': np.zeros((1, 10), np.float32), **extra},
                        os.path.join(exp, sub, f"Pred_{n}.pt"))
    ds = I.InternetDataset(None, root=str(root), device="cpu")
    mk = lambda: Renderer(faces=faces, device="cpu")
    paths = I.compose_scenes(ds, exp, renderer=mk())
    assert paths == [os.path.join(exp, "scene", "vid", f"{f:06d}.png") for f in range(2)] and not os.path.exists(os.path.join(exp, "scene_smooth"))
    assert I.scene_path(exp, "vid/000000.png") == paths[0]
    plain = [open(p, "rb").read() for p in paths]
    (pv, pcam, _), = I.scene_meshes(ds, exp, [0], W, H)
    assert np.array_equal(pv, verts) and pcam.shape == (4,)
    (sv, scam, _), = I.scene_meshes(ds, exp, [0], W, H, result_dir="result_smooth")
    assert np.array_equal(sv, verts * np.float32(0.8)) and np.array_equal(scam, np.array([0.3, 0.4, 0.2, -0.1], np.float32)) and not np.array_equal(scam, pcam)
    smooth = I.compose_scenes(ds, exp, renderer=mk(), result_dir="result_smooth", out_dir="scene_smooth")
    assert smooth == [os.path.join(exp, "scene_smooth", "vid", f"{f:06d}.png") for f in range(2)]
    assert [open(p, "rb").read() for p in paths] == plain and open(smooth[0], "rb").read() != plain[0]
    want = Renderer(resolution=(W, H), faces=faces, device="cpu").render(ds.read_frame("vid/000000.png"), sv, scam, color=I.scene_meshes(ds, exp, [0], W, H)[0][2])
    assert np.array(Image.open(smooth[0]).convert("RGB")).tobytes() == np.asarray(want).tobytes()
    assert I.frame_ids_of(ds, [[0, 1]]) == [[0, 1]]


# ------------------------------------------------------------------------------------------------ the 3DPW pass
def test_pw3d_pass_writes_its_files_and_reduces_the_acceleration_error(emu_lib, bundle, tmp_path):
    """Dumps from the noisy recipe, the clean trajectory as the dataset's ground truth (neutral tables for all three models, so the
    only error is the noise): two files, smoothed.accel < raw.accel, the line."""
    from dynaboa_amd import constants, smooth as S
    from dynaboa_amd.smpl import SMPL
    lengths = (12, 2, 9)
    x = SM.make_inputs(lengths, seed=51)
    n = sum(lengths)
    exp = str(tmp_path / "run")
    write_dumps(os.path.join(exp, "result"), range(n), x, {i: i for i in range(n)})
    smpl = SMPL(tables=bundle.smpl_neutral)
    off = SM.offsets_of(lengths)
    sequences = [list(range(off[s], off[s + 1])) for s in range(3)]
    gt_betas = np.repeat([x["betas"][off[s]:off[s + 1]].mean(0) if m else np.zeros(10) for s, m in enumerate(lengths)], lengths, axis=0)
    blocks = S.smooth_metrics(exp, sequences, ["a", "b", "c"], x["clean_aa"].reshape(n, 72), gt_betas, np.zeros(n, np.int64), smpl, smpl, smpl,
                              torch.from_numpy(bundle.smpl_neutral["J_regressor_h36m"]).float(), list(constants.H36M_TO_J14),
                              half_window=4, sigma=2.0)
    assert sorted(os.listdir(exp)) == ["metrics_per_sequence_smoothed.csv", "metrics_smoothed.json", "result"]
    m = json.load(open(os.path.join(exp, "metrics_smoothed.json")))
    assert m["half_window"] == 4 and m["sigma"] == 2.0 and m["sequences"] == 3
    for key in ("raw", "smoothed"):
        assert set(m[key]) == {"overall", "sequence_mean"} and m[key] == blocks[key]
        assert set(m[key]["overall"]) == {"frames", "mpjpe", "pampjpe", "pck", "auc", "accel", "triples"}
        assert set(m[key]["sequence_mean"]) == {"mpjpe", "pampjpe", "pck", "auc", "accel"}
        assert m[key]["overall"]["frames"] == n and m[key]["overall"]["triples"] == 10 + 0 + 7
    print("accel", m["raw"]["overall"]["accel"], "->", m["smoothed"]["overall"]["accel"])
    assert 0 < m["smoothed"]["overall"]["accel"] < m["raw"]["overall"]["accel"]
    rows = list(csv.DictReader(open(os.path.join(exp, "metrics_per_sequence_smoothed.csv"))))
    assert sorted(r["name"] for r in rows) == ["a", "b", "c"] and {"accel", "accel_raw", "pampjpe", "triples"} <= set(rows[0])
    pa = [float(r["pampjpe"]) for r in rows]
    assert pa == sorted(pa, reverse=True)
    for r in rows:
        if int(r["triples"]):
            assert float(r["accel"]) < float(r["accel_raw"])
    line = S.smoothed_line(blocks)
    assert line.startswith(f"ACCEL: {m['raw']['overall']['accel']} -> {m['smoothed']['overall']['accel']}, MPJPE: ") and ", PAMPJPE: " in line
    o = S._make_parser().parse_args(["--batch_size", "2"])
    with pytest.raises(ValueError, match="batch-size-1"):
        S.run_pw3d(o, device="cpu")


# ------------------------------------------------------------------------------------------------ on the device
SHORT = ["--inner_step", "1", "--interval", "2", "--optim_steps", "2"]


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """The g10 detections of the first six frames over 1280 x 720 frames (the tree of tests/test_scene_compose.py, one frame more)."""
    from PIL import Image
    from dynaboa_amd import internet as I
    root = tmp_path_factory.mktemp("video")
    with open(os.path.join(GOLDEN, "g10_internet_detections.json")) as fh:
        dets = [d for d in json.load(fh) if d["image_id"] in [f"{f:06d}.png" for f in range(6)]]
    with open(root / "g10seq.json", "w") as fh:
        json.dump(dets, fh)
    os.makedirs(root / "images" / "g10seq")
    yy, xx = np.mgrid[0:720, 0:1280]
    for f in range(6):
        img = np.stack([(xx // 5 + 9 * f) % 256, (yy // 3 + 5 * f) % 256, ((xx + yy) // 7 + 3 * f) % 256], -1).astype(np.uint8)
        Image.fromarray(img).save(root / "images" / "g10seq" / f"{f:06d}.png")
    I.main(["--extract", str(root)])
    return root


def _drive(folder, exp, bundle, *flags):
    from dynaboa_amd import internet as I
    o = I.parser.parse_args(["--internet_root", str(folder), "--expdir", str(exp), "--expname", "run", "--split_tracks", "1", "--scene_overlays", "1",
                             *SHORT, *flags])
    rows = I.run_driver(o, assets_bundle=bundle, device=torch.device("cuda:0"))
    torch.cuda.synchronize()
    return rows, os.path.join(str(exp), "run")


def _tree(path):
    return {os.path.relpath(os.path.join(d, f), path): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(path) for f in fs}


@pytest.mark.gpu
def test_internet_driver_with_smooth_window_gpu(folder, bundle, tmp_path):
    """--smooth_window 2 --scene_overlays 1 on six frames: result/ and scene/ are byte-equal to a run without the flag, which writes
    neither result_smooth/ nor scene_smooth/; the smoothed dumps equal smooth_results' rule on the plain ones."""
    import joblib
    from dynaboa_amd import _lib, internet as I
    assert _lib.load()._name == _lib.LIB_PATH
    rows0, run0 = _drive(folder, tmp_path / "off", bundle)
    rows1, run1 = _drive(folder, tmp_path / "on", bundle, "--smooth_window", "2")
    assert sorted(rows0) == sorted(rows1)
    assert not os.path.exists(os.path.join(run0, "result_smooth")) and not os.path.exists(os.path.join(run0, "scene_smooth"))
    for sub in ("result", "scene"):
        a, b = _tree(os.path.join(run0, sub)), _tree(os.path.join(run1, sub))
        assert sorted(a) == sorted(b) and all(a[k] == b[k] for k in a), sub
    assert sorted(os.listdir(os.path.join(run1, "result_smooth"))) == sorted(os.listdir(os.path.join(run1, "result")))
    assert sorted(_tree(os.path.join(run1, "scene_smooth"))) == sorted(_tree(os.path.join(run1, "scene")))
    ds = I.InternetDataset(None, root=str(folder), device="cpu", split_tracks=1)
    changed = 0
    for s in ds.sequences:
        src = [joblib.load(os.path.join(run1, "result", f"Pred_{n}.pt")) for n in s["rows"]]
        out = [joblib.load(os.path.join(run1, "result_smooth", f"Pred_{n}.pt")) for n in s["rows"]]
        ids = I.frame_ids_of(ds, [s["rows"]])[0]
        ref = SM.ref_smooth(np.stack([d["rotmat"].reshape(24, 9) for d in src]), np.stack([d["beta"].reshape(10) for d in src]), None,
                            (len(src),), SM.gaussian(2), 2, frame_id=ids)
        for k, (d, e) in enumerate(zip(src, out)):
            assert sorted(e) == ["beta", "cam", "cam_frame", "rotmat", "verts"] and e["cam"].tobytes() == d["cam"].tobytes()
            SM.check((e["rotmat"].reshape(1, 24, 9), e["beta"], None), [ref[0][k:k + 1], ref[1][k:k + 1], None])
            changed += int(not np.array_equal(e["rotmat"], d["rotmat"]))
    assert changed >= 6
    assert any(_tree(os.path.join(run1, "scene_smooth"))[k] != v for k, v in _tree(os.path.join(run1, "scene")).items())


@pytest.mark.gpu
def test_online_adaptor_with_one_euro_gpu(bundle):
    """--one_euro 1 over 4 frames: the unsmoothed keys equal a run without the flag; the smoothed keys equal OneEuro applied to them
    by hand (the frame camera: convert_crop_cam_to_orig_img of the frame's crop camera and box)."""
    from dynaboa_amd import _lib, assets, online as ON
    from dynaboa_amd.render import convert_crop_cam_to_orig_img
    from dynaboa_amd.smooth import OneEuro
    assert _lib.load()._name == _lib.LIB_PATH
    dev = torch.device("cuda:0")
    mk = lambda **kw: ON.OnlineAdaptor(ON.online_options(use_boa=1, log_frames=8, **kw), bundle, device=dev)
    plain, filt = mk(), mk(one_euro=1, one_euro_min_cutoff=0.8, one_euro_beta=0.3, fps=25.0)
    assert plain.one_euro is None and filt.one_euro is not None
    hand = OneEuro(1, fps=25.0, min_cutoff=0.8, beta=0.3, J=24, nb=10, nc=4, device=dev)
    size = (320, 240)
    for n in range(4):
        fr = {k: v.to(dev) for k, v in assets.make_online_frame(n, seed=22).items()}
        bbox = torch.tensor([[150.0 + 2 * n, 120.0 - n, 140.0 + 3 * n]], device=dev)
        a = {k: v.clone() for k, v in plain.adapt_processed(fr["image"], fr["smpl_j2d"], bbox).items()}
        b = filt.adapt_processed(fr["image"], fr["smpl_j2d"], bbox, frame_size=size)
        assert set(b) == set(a) | {"vts_smooth", "rotmat_smooth", "shape_smooth", "cam_frame_smooth"}
        for k in a:
            assert torch.equal(a[k], b[k]), (n, k)
        camf = convert_crop_cam_to_orig_img(b["cam"].detach().float(), bbox, *size)
        R, S, Cf = hand.step(b["rotmat"], b["shape"], camf)
        assert torch.equal(R, b["rotmat_smooth"]) and torch.equal(S, b["shape_smooth"]) and torch.equal(Cf, b["cam_frame_smooth"])
        with torch.no_grad():
            v = filt.decode_smpl_params(R, S)["vts"]
        assert torch.equal(v, b["vts_smooth"])
        if n == 0:
            assert torch.equal(b["rotmat_smooth"], b["rotmat"]) and torch.equal(b["vts_smooth"], b["vts"])
        else:
            assert not torch.equal(b["rotmat_smooth"], b["rotmat"])
    frame = torch.zeros(size[1], size[0], 3, dtype=torch.uint8, device=dev)
    pic, pic_s = filt.render(b, frame), filt.render(b, frame, smooth=True)
    assert pic.shape == pic_s.shape == (size[1], size[0], 3) and not torch.equal(pic, pic_s)
    with pytest.raises(ValueError):
        plain.render(a, frame, smooth=True)
    c = filt.adapt_processed(fr["image"], fr["smpl_j2d"])                  # no box: no camera key
    assert "cam_frame_smooth" not in c and "vts_smooth" in c


@pytest.mark.gpu
def test_online_group_runs_one_filter_over_its_sequences_gpu(bundle):
    """Two sequences in an OnlineGroup with --one_euro 1, two steps: one filter of two rows, equal to OneEuro(2) applied by hand; the
    adaptors' own filters are not stepped."""
    from dynaboa_amd import _lib, assets, online as ON
    from dynaboa_amd.render import convert_crop_cam_to_orig_img
    from dynaboa_amd.smooth import OneEuro
    assert _lib.load()._name == _lib.LIB_PATH
    dev = torch.device("cuda:0")
    ads = [ON.OnlineAdaptor(ON.online_options(use_boa=1, log_frames=8, one_euro=1), bundle, device=dev) for _ in range(2)]
    grp = ON.OnlineGroup(ads)
    assert grp.one_euro is not None and grp.one_euro.state.shape[0] == 2
    hand = OneEuro(2, J=24, nb=10, nc=4, device=dev)
    size = (320, 240)
    for n in range(2):
        items = []
        for r in range(2):
            fr = {k: v.to(dev) for k, v in assets.make_online_frame(n + 100 * r, seed=22).items()}
            items.append((fr["image"], fr["smpl_j2d"], torch.tensor([[150.0 + n, 120.0 + 5 * r, 140.0]], device=dev), size))
        out = grp.step_processed(items)
        camf = torch.cat([convert_crop_cam_to_orig_img(o["cam"].detach().float(), it[2], *size) for o, it in zip(out, items)])
        R, S, Cf = hand.step(torch.cat([o["rotmat"] for o in out]), torch.cat([o["shape"] for o in out]), camf)
        for r, o in enumerate(out):
            assert torch.equal(o["rotmat_smooth"], R[r:r + 1]) and torch.equal(o["shape_smooth"], S[r:r + 1])
            assert torch.equal(o["cam_frame_smooth"], Cf[r:r + 1]) and o["vts_smooth"].shape == (1, 6890, 3)
            assert torch.equal(o["vts_smooth"], o["vts"]) == (n == 0)
    assert torch.equal(grp.one_euro.state, hand.state) and not ads[0].one_euro.state.any()
