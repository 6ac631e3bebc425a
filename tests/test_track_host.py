"""The tracker's host side: dynaboa_amd.track (track_videos, the command line), ``internet --extract --track 1`` and the online driver's
``--track 1`` on the emulator library with CPU tensors (the `emu_lib` pattern of tests/test_smooth_host.py); marked gpu, the online
driver with --track 1 on cuda:0."""
import ctypes
import json
import os
import zipfile

import numpy as np
import pytest
import torch

import track_cases as TR
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


# ------------------------------------------------------------------------------------------------ track_videos
def test_track_videos_nesting_and_counts(emu_lib):
    """The scene beside an empty video and a short one: the outputs nest as the inputs do and equal the restatement."""
    from dynaboa_amd.track import track_videos
    scene, _ = TR.make_scene()
    a = TR.person(200, 300, K=TR.SCENE_K)
    videos = [scene, [], [a[None], np.zeros((0, TR.SCENE_K, 3), np.float32), np.stack([a, a])]]
    tracks, sims, counts = track_videos(videos, device="cpu")
    assert [len(v) for v in tracks] == [60, 0, 3] == [len(v) for v in sims] and len(counts) == 3
    rt, rs, rv = TR.ref_track(*TR.pack(videos), **TR.RULE)
    assert np.array_equal(np.concatenate([t for v in tracks for t in v]), rt)
    assert all(t.dtype == np.int32 and s.dtype == np.float32 and t.shape == s.shape == (f.shape[0],)
               for v, tv, sv in zip(videos, tracks, sims) for f, t, s in zip(v, tv, sv))
    assert np.abs(np.concatenate([s for v in sims for s in v]) - rs).max() <= TR.BOUND
    assert counts == [dict(started=7, untrackable=1, no_slot=0), dict(started=0, untrackable=0, no_slot=0), dict(started=2, untrackable=0, no_slot=0)]
    assert [t.tolist() for t in tracks[2]] == [[0], [], [0, 1]]
    # frame ids and the rule's keywords reach the kernel
    tracks, _, _ = track_videos([[a[None]] * 3], [[0, 1, 9]], device="cpu")
    assert [t.tolist() for t in tracks[0]] == [[0], [0], [1]]
    tracks, _, _ = track_videos([[a[None]] * 3], [[0, 1, 9]], max_age=8, device="cpu")
    assert [t.tolist() for t in tracks[0]] == [[0], [0], [0]]
    assert track_videos([], device="cpu") == ([], [], [])
    tracks, sims, counts = track_videos([[]], device="cpu")
    assert tracks == [[]] and counts == [dict(started=0, untrackable=0, no_slot=0)]


def test_track_videos_value_errors(emu_lib):
    from dynaboa_amd.track import track_videos
    a = TR.person(200, 300, K=5)
    with pytest.raises(ValueError, match="one K"):
        track_videos([[a[None], TR.person(200, 300, K=6)[None]]], device="cpu")
    with pytest.raises(ValueError, match="increase"):
        track_videos([[a[None]] * 3], [[0, 2, 2]], device="cpu")
    with pytest.raises(ValueError, match="one id per frame"):
        track_videos([[a[None]] * 3], [[0, 1]], device="cpu")
    with pytest.raises(ValueError, match="outside"):
        track_videos([[np.zeros((1, 33, 3), np.float32)]], device="cpu")
    crowd = TR.grid(65)
    with pytest.raises(ValueError, match="65 detections"):
        track_videos([[crowd]], strict=True, device="cpu")
    tracks, _, counts = track_videos([[crowd]], device="cpu")                   # strict=False: the kernel's rule
    assert tracks[0][0].tolist() == list(range(64)) + [-1] and counts[0]["no_slot"] == 1
    with pytest.raises(RuntimeError, match="dyb_track_videos"):
        track_videos([[a[None]]], kappa=0.0, device="cpu")


# ------------------------------------------------------------------------------------------------ the command line
def body25(rng):
    return np.stack([rng.uniform(-25, 25, 25), rng.uniform(-40, 40, 25)], -1)


def write_openpose(folder, frames_dir, n_frames, swap_from, size=(160, 120), seed=4):
    """Two people, A around x = 40 and B around x = 115, drifting one pixel per frame; from frame `swap_from` on OpenPose lists B
    first.  Frames <frames_dir>/f_<i>.png, detections <folder>/f_<i>_keypoints.json.  -> (names, per frame [A's kp, B's kp])."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(folder), os.makedirs(frames_dir)
    tpl = [body25(rng) + c for c in ((40.0, 60.0), (115.0, 60.0))]
    names, truth = [], []
    for i in range(n_frames):
        kps = [np.concatenate([t + (i, 0.5 * i) + rng.normal(0, 0.3, (25, 2)), rng.uniform(0.4, 1.0, (25, 1))], -1).astype(np.float32) for t in tpl]
        order = kps[::-1] if i >= swap_from else kps
        with open(os.path.join(folder, f"f_{i:04d}_keypoints.json"), "w") as fh:
            json.dump(dict(version=1.3, people=[dict(pose_keypoints_2d=[float(v) for v in k.reshape(-1)]) for k in order]), fh)
        Image.fromarray(rng.integers(0, 255, (size[1], size[0], 3), dtype=np.uint8)).save(os.path.join(frames_dir, f"f_{i:04d}.png"))
        names.append(f"f_{i:04d}.png"); truth.append(kps)
    return names, truth


def test_command_line_keeps_one_person_per_file_where_people0_does_not(emu_lib, tmp_path):
    from dynaboa_amd import online as ON, track as T
    names, truth = write_openpose(str(tmp_path / "op"), str(tmp_path / "frames"), 10, swap_from=5)
    with open(tmp_path / "op" / "f_0007_keypoints.json") as fh:
        rec = json.load(fh)
    rec["people"].append(dict(pose_keypoints_2d=[0.0] * 75))                    # an all-zero person: untrackable, in no file
    with open(tmp_path / "op" / "f_0007_keypoints.json", "w") as fh:
        json.dump(rec, fh)
    paths = T.main(["--openpose", str(tmp_path / "op"), "--frames", str(tmp_path / "frames"), "--out", str(tmp_path / "out")], device="cpu")
    assert sorted(os.listdir(tmp_path / "out")) == ["track0.npz", "track1.npz", "tracks.json"] and sorted(paths) == [0, 1]
    for t in (0, 1):
        z = np.load(paths[t], allow_pickle=False)
        assert z["imgname"].tolist() == names and z["keypoints"].shape == (10, 25, 3) and z["keypoints"].dtype == np.float32
        assert all(np.array_equal(z["keypoints"][i], truth[i][t]) for i in range(10))            # one person throughout
        dets = ON.load_detections(paths[t], names)                                               # what --detections FILE reads
        assert sorted(dets) == names and np.array_equal(dets[names[6]], truth[6][t])
    first = ON.load_detections(str(tmp_path / "op"), names)                                      # people[0]: the defect this closes
    assert np.array_equal(first[names[4]], truth[4][0]) and np.array_equal(first[names[5]], truth[5][1])
    info = json.load(open(tmp_path / "out" / "tracks.json"))
    assert info["tracks"] == [dict(id=t, first=names[0], last=names[9], frames=10) for t in (0, 1)]
    assert info["counts"] == dict(started=2, untrackable=1, no_slot=0) and info["frames"] == 10
    # --min_track_frames drops the short track; without --frames imgname holds the stems; the rule flags reach the kernel
    os.remove(tmp_path / "op" / "f_0003_keypoints.json")
    os.remove(tmp_path / "op" / "f_0004_keypoints.json")
    paths = T.main(["--openpose", str(tmp_path / "op"), "--out", str(tmp_path / "out2"), "--max_age", "1", "--min_track_frames", "4"], device="cpu")
    assert sorted(paths) == [2, 3] and np.load(paths[2])["imgname"].tolist() == [f"f_{i:04d}" for i in range(5, 10)]
    assert [r["frames"] for r in json.load(open(tmp_path / "out2" / "tracks.json"))["tracks"]] == [5, 5]
    assert T.read_openpose(str(tmp_path / "op"))[2] == [0, 1, 2, 5, 6, 7, 8, 9]                  # frame ids from the stems


def test_parser_defaults_are_off():
    from dynaboa_amd import internet as I, online as ON, track as T
    rule = dict(c_min=T.C_MIN, kappa=T.KAPPA, s_min=T.S_MIN, max_age=T.MAX_AGE, min_common=T.MIN_COMMON)
    for o in (I.parser.parse_args([]), ON.parser.parse_args([]), ON.online_options()):
        assert o.track == 0 and T.rule_of(o) == rule
    o = T._make_parser().parse_args(["--openpose", "a", "--out", "b"])
    assert T.rule_of(o) == rule and o.min_track_frames == 1 and o.frames is None
    assert ON.parser.parse_args([]).min_track_frames == 1


def test_online_track_refuses_a_file_and_a_given_adaptor(tmp_path):
    from dynaboa_amd import online as ON
    (tmp_path / "frames").mkdir()
    np.savez(tmp_path / "det.npz", imgname=np.array([]), keypoints=np.zeros((0, 25, 3), np.float32))
    o = ON.online_options(track=1, frames=str(tmp_path / "frames"), detections=str(tmp_path / "det.npz"), out=str(tmp_path / "out"))
    with pytest.raises(ValueError, match="directory of OpenPose"):
        ON.run_driver(o, device="cpu")
    (tmp_path / "op").mkdir()
    o.detections = str(tmp_path / "op")
    with pytest.raises(ValueError, match="fresh adaptation state"):
        ON.run_driver(o, adaptor=object(), device="cpu")
    assert not os.path.exists(tmp_path / "out")


def test_online_track_hands_every_track_to_the_loop_alone(emu_lib, tmp_path, monkeypatch):
    """--track 1 with the adaptor and the frame loop replaced by recorders: the tracker's files are written, every kept track gets
    an adaptor of its own and its own detections, one after the other, into <out>/track<id>."""
    from dynaboa_amd import online as ON
    names, truth = write_openpose(str(tmp_path / "op"), str(tmp_path / "frames"), 6, swap_from=3)
    made, calls = [], []
    monkeypatch.setattr(ON, "OnlineAdaptor", lambda *a, **k: (made.append(len(made)), made[-1])[1])
    monkeypatch.setattr(ON, "drive_frames", lambda o, nm, dets, ad, out: (calls.append((ad, out, dets, list(nm))), [out])[1])
    o = ON.online_options(track=1, frames=str(tmp_path / "frames"), detections=str(tmp_path / "op"), out=str(tmp_path / "out"))
    written = ON.run_driver(o, device="cpu")
    assert written == [str(tmp_path / "out" / "track0"), str(tmp_path / "out" / "track1")] and made == [0, 1]
    assert sorted(os.listdir(tmp_path / "out")) == ["track0.npz", "track1.npz", "tracks.json"]
    for t, (ad, out, dets, nm) in enumerate(calls):
        assert ad == t and nm == names and sorted(dets) == names
        assert all(np.array_equal(dets[n], truth[i][t]) for i, n in enumerate(names))


# ------------------------------------------------------------------------------------------------ internet --extract
def parent_extract(in_path, seq, out_file):
    """The extraction as it stood before --track (reference utils/data_preprocess/internet_data.py:42-79), restated."""
    from dynaboa_amd import constants as C, internet as I
    with open(os.path.join(in_path, f"{seq}.json")) as fh:
        annots = json.load(fh)
    imagenames, scales, centers, j2ds, tracks = [], [], [], [], []
    for annot in annots:
        kps2d = np.array(annot['keypoints']).reshape(-1, 3)
        if annot['score'] < I.MIN_SCORE or I.person_height(kps2d) < I.MIN_HEIGHT:
            continue
        center, scale = I.detection_bbox(kps2d)
        kps2d[:, 2] = kps2d[:, 2] > I.CONF_THRESHOLD
        part = np.zeros([C.NUM_OUT_JOINTS, 3])
        part[list(I.COCO_TO_49)] = kps2d
        imagenames.append(os.path.join(seq, annot['image_id']))
        centers.append(center); scales.append(scale); j2ds.append(part); tracks.append(I.track_of(annot))
    np.savez(out_file, imgname=imagenames, center=centers, scale=scales, part=j2ds, track=np.array(tracks, dtype=np.int64))


def members(path):
    with zipfile.ZipFile(path) as z:
        return [(n, z.read(n)) for n in z.namelist()]


def test_extract_without_track_writes_the_parents_bytes(tmp_path, monkeypatch):
    """--track 0 (the default): every member of <seq>.npz - names, order, bytes - is what the extraction wrote before the flag
    existed, and the tracker is not touched.  (The archive's own header carries the time of writing: the members are compared.)"""
    import shutil
    from dynaboa_amd import internet as I, track as T
    monkeypatch.setattr(T, "track_videos", lambda *a, **k: pytest.fail("the tracker ran"))
    shutil.copy(os.path.join(GOLDEN, "g10_internet_detections.json"), tmp_path / "vid.json")
    I.main(["--extract", str(tmp_path)])
    parent_extract(str(tmp_path), "vid", str(tmp_path / "parent.npz"))
    got, want = members(tmp_path / "vid.npz"), members(tmp_path / "parent.npz")
    assert [n for n, _ in got] == ["imgname.npy", "center.npy", "scale.npy", "part.npy", "track.npy"] and got == want


def alphapose_records(seed=8, frames=8, with_idx=False):
    """Three people of 120 x 330 pixels over `frames` frames as AlphaPose records, the records of the whole file shuffled.
    -> (records, person of every record)."""
    rng = np.random.default_rng(seed)
    tpl = [np.stack([rng.uniform(-60, 60, 17), rng.uniform(-165, 165, 17)], -1) for _ in range(3)]
    for t in tpl:
        t[0], t[1] = (-60, -165), (60, 165)
    recs, who = [], []
    for f in range(frames):
        for p in range(3):
            xy = tpl[p] + (250 + 350 * p + 2 * f, 360 + f) + rng.normal(0, 0.5, (17, 2))
            kp = np.concatenate([xy, rng.uniform(0.5, 0.95, (17, 1))], -1)
            rec = dict(image_id=f"{f:06d}.png", category_id=1, keypoints=[float(v) for v in kp.reshape(-1)], score=3.0)
            if with_idx:
                rec["idx"] = [7]                                                 # one id for everybody: what --track 1 overrides
            recs.append(rec); who.append(p)
    order = rng.permutation(len(recs))
    return [recs[i] for i in order], [who[i] for i in order]


@pytest.mark.parametrize("with_idx", [False, True])
def test_extract_with_track_follows_each_person(emu_lib, tmp_path, with_idx):
    """--extract DIR --track 1 on records in shuffled order: the track array holds one id per person (records that carry idx are
    overridden), every other array is what --track 0 writes, and InternetDataset(split_tracks=1) yields one sequence per person -
    where the same file without the flag gives one sequence over all three bodies."""
    from dynaboa_amd import internet as I
    recs, who = alphapose_records(with_idx=with_idx)
    for d in ("plain", "tracked"):
        os.makedirs(tmp_path / d)
        with open(tmp_path / d / "vid.json", "w") as fh:
            json.dump(recs, fh)
    I.run_driver(I.parser.parse_args(["--extract", str(tmp_path / "plain")]), device=torch.device("cpu"))
    I.run_driver(I.parser.parse_args(["--extract", str(tmp_path / "tracked"), "--track", "1"]), device=torch.device("cpu"))
    a, b = np.load(tmp_path / "plain" / "vid.npz"), np.load(tmp_path / "tracked" / "vid.npz")
    assert a.files == b.files and all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a.files if k != "track")
    assert b["track"].dtype == np.int64 and (a["track"] == (7 if with_idx else -1)).all()
    who = np.array(who)
    ids = [set(b["track"][who == p].tolist()) for p in range(3)]
    assert all(len(s) == 1 for s in ids) and set.union(*ids) == {0, 1, 2}
    ds = I.InternetDataset(None, root=str(tmp_path / "tracked"), device="cpu", split_tracks=1)
    assert sorted(s["frames"] for s in ds.sequences) == [8, 8, 8]
    assert all(len(set(who[s["rows"]])) == 1 for s in ds.sequences)
    plain = I.InternetDataset(None, root=str(tmp_path / "plain"), device="cpu", split_tracks=1)
    assert [s["frames"] for s in plain.sequences] == [24]


def test_track_without_extract_is_refused_before_anything_is_read(tmp_path, monkeypatch):
    from dynaboa_amd import internet as I
    monkeypatch.setattr(I, "Adaptor", lambda *a, **k: pytest.fail("an adaptor was built"))
    monkeypatch.setattr(I, "InternetDataset", lambda *a, **k: pytest.fail("the dataset was read"))
    o = I.parser.parse_args(["--internet_root", str(tmp_path), "--expdir", str(tmp_path / "none"), "--expname", "run", "--track", "1"])
    with pytest.raises(ValueError, match=r"--extract DIR"):
        I.run_driver(o, device=torch.device("cpu"))
    assert not os.path.exists(tmp_path / "none")


def test_extract_with_track_is_one_call_over_all_files(emu_lib, tmp_path, monkeypatch):
    from dynaboa_amd import internet as I, track as T
    recs, who = alphapose_records()
    for name in ("a", "b"):
        with open(tmp_path / f"{name}.json", "w") as fh:
            json.dump(recs if name == "a" else recs[:9], fh)
    with open(tmp_path / "c.json", "w") as fh:
        json.dump([], fh)
    calls, inner = [], T.track_videos
    monkeypatch.setattr(T, "track_videos", lambda v, ids, **k: (calls.append((len(v), ids)), inner(v, ids, **k))[1])
    I.run_driver(I.parser.parse_args(["--extract", str(tmp_path), "--track", "1", "--max_age", "3"]), device=torch.device("cpu"))
    assert len(calls) == 1 and calls[0][0] == 3 and calls[0][1][0] == list(range(8)) and calls[0][1][2] == []
    assert np.load(tmp_path / "c.npz")["track"].shape == (0,) and len(np.load(tmp_path / "b.npz")["track"]) == 9


# ------------------------------------------------------------------------------------------------ on the device
@pytest.mark.gpu
def test_online_driver_with_track_equals_the_driver_on_each_tracks_file_gpu(tmp_path):
    """--track 1 on two synthetic people over 4 frames whose listing order swaps: <out>/track0/ and <out>/track1/ hold the arrays, to
    the byte, of two runs of the unchanged driver on track0.npz and track1.npz."""
    from dynaboa_amd import _lib, online as ON
    from dynaboa_amd.base_adaptor import synthetic_bundle
    assert _lib.load()._name == _lib.LIB_PATH
    names, truth = write_openpose(str(tmp_path / "op"), str(tmp_path / "frames"), 4, swap_from=2)
    bundle = lambda: synthetic_bundle(seed=22, identity_pose=False, randomize_norm=True, smpl_seed=0)
    opts = dict(use_boa=1, interval=2, log_frames=4, frames=str(tmp_path / "frames"))
    o = ON.online_options(track=1, detections=str(tmp_path / "op"), out=str(tmp_path / "out"), **opts)
    written = ON.run_driver(o, assets_bundle=bundle(), device="cuda:0")
    assert [os.path.relpath(p, tmp_path / "out") for p in written] == [f"track{t}/Pred_{n}.npz" for t in (0, 1) for n in range(4)]
    for t in (0, 1):
        z = np.load(tmp_path / "out" / f"track{t}.npz")
        assert all(np.array_equal(z["keypoints"][i], truth[i][t]) for i in range(4))
        alone = ON.run_driver(ON.online_options(detections=str(tmp_path / "out" / f"track{t}.npz"), out=str(tmp_path / f"alone{t}"), **opts),
                              assets_bundle=bundle(), device="cuda:0")
        for n, p in enumerate(alone):
            a, b = np.load(p), np.load(tmp_path / "out" / f"track{t}" / f"Pred_{n}.npz")
            assert a.files == b.files and all(a[k].tobytes() == b[k].tobytes() and a[k].shape == b[k].shape for k in a.files)
    a, b = np.load(tmp_path / "out" / "track0" / "Pred_3.npz"), np.load(tmp_path / "out" / "track1" / "Pred_3.npz")
    assert not np.array_equal(a["verts"], b["verts"])
