"""The host side of the internet-video path (dynaboa_amd/internet.py) against the reference's own code, recorded by
tools/make_golden_internet.py: detections -> npz (``internet_data_extract``), dataset items (``Internet_dataset``), the track
sequences of ``--split_tracks`` and the lockstep group loader (crops on the kernel emulator)."""
import ctypes
import json
import os
import shutil

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden

SEQ = "g10seq"


@pytest.fixture(scope="module")
def emu_lib():
    from emu.build_emu import build
    from dynaboa_amd import _abi, _lib
    lib = _abi.bind(ctypes.CDLL(build()))
    saved = _lib._lib
    _lib.use_library(lib)
    yield lib
    _lib._lib = saved


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """<root>/g10seq.json, extracted; a second, smaller file 'a_first' that sorts in front of it."""
    from dynaboa_amd import internet as I
    root = tmp_path_factory.mktemp("internet")
    shutil.copy(os.path.join(GOLDEN, "g10_internet_detections.json"), root / f"{SEQ}.json")
    with open(os.path.join(GOLDEN, "g10_internet_detections.json")) as fh:
        dets = json.load(fh)
    first = [dict(d, image_id="x_" + d["image_id"]) for d in dets if d["image_id"] in ("000000.png", "000001.png")]
    with open(root / "a_first.json", "w") as fh:
        json.dump(first, fh)
    written = I.internet_data_extract(str(root))
    assert [os.path.basename(w) for w in written] == ["a_first.npz", f"{SEQ}.npz"]
    return root


def test_extract_equals_the_reference(folder):
    g = golden("g10_internet_extract.npz")
    z = np.load(folder / f"{SEQ}.npz")
    assert sorted(z.files) == sorted(list(g.files) + ["track"])
    for k in g.files:
        assert z[k].dtype == g[k].dtype and z[k].shape == g[k].shape and np.array_equal(z[k], g[k]), k
    # 8 rows of track 0, 5 of track 1 (its frame 3 fails the score test), the two of frame 7: one without idx, one with a scalar idx
    want = {}
    for name, tr in zip(z["imgname"], z["track"]):
        want.setdefault(int(tr), []).append(str(name))
    assert z["track"].dtype == np.int64 and {k: len(v) for k, v in want.items()} == {0: 8, 1: 5, -1: 1, 5: 1}
    assert os.path.join(SEQ, "000003.png") not in want[1] and want[-1] == [os.path.join(SEQ, "000007.png")]
    part = z["part"]
    assert float(np.abs(part[:, :25]).sum()) == 0.0                                  # all 17 joints land in the gt24 window
    assert (np.abs(part[:, 25:, :2]).sum(-1) == 0).sum(1).tolist() == [7] * len(part)  # ... 7 of whose 24 joints stay exact zeros
    assert set(np.unique(part[:, :, 2])) == {0.0, 1.0} and (part[:, 25:, 2] == 0).sum() > 7 * len(part)     # thresholded; some joints below 0.3


def test_extract_command_line(folder, tmp_path):
    from dynaboa_amd import internet as I
    shutil.copy(folder / f"{SEQ}.json", tmp_path / f"{SEQ}.json")
    I.main(["--extract", str(tmp_path)])
    a, b = np.load(tmp_path / f"{SEQ}.npz"), np.load(folder / f"{SEQ}.npz")
    assert all(np.array_equal(a[k], b[k]) for k in b.files)


def test_dataset_items_equal_the_reference(folder):
    from dynaboa_amd import internet as I
    g = golden("g10_internet_items.npz")
    ds = I.InternetDataset(None, root=str(folder), device="cpu", files=[str(folder / f"{SEQ}.npz")])
    assert len(ds) == len(g["bbox"]) == 15 and ds.img_dir == os.path.join(str(folder), "images")
    stored = ds.smpl_j2ds.copy()
    for rep in range(2):                                 # a second read gives the same item: the stored keypoints are not rewritten
        for i in range(len(ds)):
            h = ds.annotations(i)
            assert h["smpl_j2d"].dtype == np.float32 and np.array_equal(h["smpl_j2d"], g["smpl_j2d"][i]), (rep, i)
            assert np.array_equal(np.array([h["center"][0], h["center"][1], h["scale"] * 200]), g["bbox"][i]), (rep, i)
            assert h["imgname"] == str(ds.imgnames[i]) and h["row"] == i
    assert np.array_equal(ds.smpl_j2ds, stored)


def test_sequences_default_and_split(folder):
    from dynaboa_amd import internet as I
    ds = I.InternetDataset(None, root=str(folder), device="cpu")
    assert [os.path.basename(f) for f in ds.files] == ["a_first.npz", f"{SEQ}.npz"]           # sorted, not glob order
    n0 = 4                                                                                        # a_first: frames 0, 1 of tracks 0 and 1
    assert len(ds) == n0 + 15
    assert ds.sequences == [dict(file=None, track=None, first=0, frames=19, rows=list(range(19)))]
    sp = I.InternetDataset(None, root=str(folder), device="cpu", split_tracks=1)
    key = [(os.path.basename(s["file"]), s["track"], s["frames"]) for s in sp.sequences]
    assert key == [("a_first.npz", 0, 2), ("a_first.npz", 1, 2), (f"{SEQ}.npz", 0, 8), (f"{SEQ}.npz", 1, 5), (f"{SEQ}.npz", -1, 1),
                   (f"{SEQ}.npz", 5, 1)]                                                        # per file, order of first appearance
    for s in sp.sequences:
        assert s["first"] == s["rows"][0] and s["rows"] == sorted(s["rows"]) and len(s["rows"]) == s["frames"]
        assert all(int(sp.tracks[r]) == s["track"] and sp.files[int(sp.file_of[r])] == s["file"] for r in s["rows"])
    rows = [r for s in sp.sequences for r in s["rows"]]
    assert sorted(rows) == list(range(19))              # every row in exactly one sequence: Pred_{row} is unique under split
    sp3 = I.InternetDataset(None, root=str(folder), device="cpu", split_tracks=1, min_track_frames=3)
    assert [(s["track"], s["frames"]) for s in sp3.sequences] == [(0, 8), (1, 5)]
    # options stand in for the keyword arguments (what BaseAdaptor.set_dataloader passes)
    o = type("O", (), dict(internet_root=str(folder), split_tracks=1, min_track_frames=5))()
    assert [(s["track"], s["frames"]) for s in I.InternetDataset(o, device="cpu").sequences] == [(0, 8), (1, 5)]


def _write_frames(folder, ds, size=(90, 160)):
    from PIL import Image
    rng = np.random.default_rng(3)
    for name in sorted(set(str(n) for n in ds.imgnames)):
        p = os.path.join(ds.img_dir, name)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        if not os.path.exists(p):
            Image.fromarray(rng.integers(0, 256, size + (3,), dtype=np.uint8)).save(p)


def test_group_loader_shares_frames_and_matches_items(emu_lib, folder, monkeypatch):
    """Lockstep walk of the two long tracks: a sequence that ends early leaves the step list, a frame two tracks share is decoded once,
    the crops (one preprocess_frames call per step) equal the single-item path bit for bit.  (Frames 160 x 90: the detections were
    made for 1280 x 720, so every box hangs over the frame - the crop does not care.)"""
    from dynaboa_amd import datasets as D, internet as I
    ds = I.InternetDataset(None, root=str(folder), device="cpu", files=[str(folder / f"{SEQ}.npz")], split_tracks=1, min_track_frames=3)
    _write_frames(folder, ds)
    reads, calls = [], []
    real_read, real_many = D.read_image, D.preprocess_frames
    monkeypatch.setattr(D, "read_image", lambda p: (reads.append(os.path.basename(p)), real_read(p))[1])
    monkeypatch.setattr(D, "preprocess_frames", lambda *a, **k: (calls.append(len(a[0])), real_many(*a, **k))[1])
    loader = I.TrackGroupLoader(ds, ds.sequences, workers=2)
    steps = list(loader)
    assert len(loader) == len(steps) == 8
    assert [[si for si, _ in st] for st in steps] == [[0, 1]] * 5 + [[0]] * 3          # track 1 has 5 rows: it leaves after step 4
    assert calls == [2] * 5 + [1] * 3
    # track 1 misses frame 3, so from step 3 on the two tracks sit on different frames: 3 shared steps, 2 + 2 unshared, 3 single
    assert loader.decoded == len(reads) == 3 + 4 + 3
    monkeypatch.undo()
    for st in steps:
        for si, b in st:
            row = b["row"][0]
            it = ds[row]
            assert set(b) == {"image", "imgname", "smpl_j2d", "bbox", "row"} and tuple(b["image"].shape) == (1, 3, 224, 224)
            assert b["imgname"] == [it["imgname"]] and row in ds.sequences[si]["rows"]
            assert torch.equal(b["image"][0], it["image"]) and torch.equal(b["smpl_j2d"][0], it["smpl_j2d"])
            assert torch.equal(b["bbox"][0], it["bbox"]) and b["bbox"].dtype == torch.float64
    unbatched = list(I.TrackGroupLoader(ds, ds.sequences, workers=1, batched=False))
    assert all(torch.equal(a[1]["image"], b[1]["image"]) for sa, sb in zip(steps, unbatched) for a, b in zip(sa, sb))


def test_set_dataloader_builds_the_internet_stream(emu_lib, folder):
    """BaseAdaptor.set_dataloader with --dataset internet: the reference's single stream, batches in the reference's schema."""
    from dynaboa_amd import benchmark as DB, internet as I
    from dynaboa_amd.base_adaptor import BaseAdaptor
    ds0 = I.InternetDataset(None, root=str(folder), device="cpu")
    _write_frames(folder, ds0)
    a = BaseAdaptor.__new__(BaseAdaptor)
    a.options = DB.parser.parse_args(["--dataset", "internet"])
    a.options.internet_root = str(folder)
    a.device, a.bundle = torch.device("cpu"), None
    a.set_dataloader()
    assert len(a.dataloader) == 19 and a.imgdir == os.path.join(str(folder), "images")
    b = next(iter(a.dataloader))
    assert tuple(b["image"].shape) == (1, 3, 224, 224) and tuple(b["smpl_j2d"].shape) == (1, 49, 3) and tuple(b["bbox"].shape) == (1, 3)
    assert b["imgname"] == [str(ds0.imgnames[0])] and b["row"] == [0]
    # the internet driver's parser has its own defaults and flags; the benchmark driver's are left as they were
    o = I.parser.parse_args([])
    assert (o.dataset, o.dump_predictions, o.native_results, o.split_tracks, o.min_track_frames, o.interval, o.seqs_per_gpu) == \
        ("internet", 1, 1, 0, 1, 5, 1)
    b0 = DB.parser.parse_args([])
    assert (b0.dataset, b0.dump_predictions, b0.native_results) == ("3dpw", 0, 0) and not hasattr(b0, "split_tracks")


def test_run_tracks_waves_numbering_and_early_leave(emu_lib, folder, monkeypatch):
    """internet.run_tracks with the stepper replaced by a recorder: waves of seqs_per_gpu sequences, longest first; every lockstep
    step hands the group one batch per live track and None for a track that has ended; result numbers are the rows - unique over
    all tracks; a wave of one sequence goes through Adaptor.excute with the same numbering; ranks split the tracks."""
    from dynaboa_amd import internet as I, native_step as NS
    ds = I.InternetDataset(None, root=str(folder), device="cpu", files=[str(folder / f"{SEQ}.npz")], split_tracks=1)
    _write_frames(folder, ds)
    log = []

    class FakeAdaptor:
        number_by_row = False

        def excute(self, frames, nframes=None):
            assert self.number_by_row
            log.append(("alone", [b["row"][0] for b in frames], nframes))

    class FakeGroup:
        def __init__(self, ads, steps):
            self.stepper = type("S", (), dict(join=lambda self: None))()
            log.append(("group", len(ads), steps))

        def step(self, batches, step, result_steps=None):
            assert all((b is None) or b["row"][0] == n for b, n in zip(batches, result_steps))
            log.append(("step", step, [None if b is None else b["row"][0] for b in batches]))

    monkeypatch.setattr(NS, "ReplicaGroup", FakeGroup)
    o = type("O", (), dict(batch_size=1, native_results=1))()
    t0, t1 = ds.sequences[0]["rows"], ds.sequences[1]["rows"]
    done = I.run_tracks(o, ds, FakeAdaptor, seqs_per_gpu=2)
    assert sorted(done) == list(range(15)) and len(set(done)) == 15
    assert log[0] == ("group", 2, 8)
    assert [l[2] for l in log[1:9]] == [[t0[s], t1[s] if s < 5 else None] for s in range(8)]
    assert log[9] == ("group", 2, 1) and log[10] == ("step", 0, [13, 14]) and len(log) == 11
    del log[:]
    done = I.run_tracks(o, ds, FakeAdaptor, seqs_per_gpu=3)
    assert log[0] == ("group", 3, 8) and log[1][2] == [t0[0], t1[0], 13] and log[2][2] == [t0[1], t1[1], None]
    assert log[-1] == ("alone", [14], 1) and sorted(done) == list(range(15))
    del log[:]
    r0 = I.run_tracks(o, ds, FakeAdaptor, num_shards=2, shard_rank=0)
    r1 = I.run_tracks(o, ds, FakeAdaptor, num_shards=2, shard_rank=1)
    assert sorted(r0 + r1) == list(range(15)) and r0 == t0 and all(l[0] == "alone" for l in log)
    o.native_results = 0
    with pytest.raises(ValueError, match="native_results"):
        I.run_tracks(o, ds, FakeAdaptor, seqs_per_gpu=2)


def test_synthetic_frame_is_coco_shaped_and_stream_goldens_cover_both_exits():
    """The frames of the stream goldens: the 17 mapped joints keep assets.make_frame's values, the 25 OpenPose slots and the 7 unmapped
    joints of the gt24 window are exact zeros.  The gated golden has a frame leaving by convergence and frames at the cut-off, every
    decision at least 2 % of the threshold away; both tags carry the Pred dictionaries and a noise file for the same tensors."""
    from dynaboa_amd import assets, internet as I
    fr, base = I.synthetic_frame(3), assets.make_frame(3, 1, seed=22)
    kp = fr["smpl_j2d"]
    mapped = sorted(I.COCO_TO_49)
    rest = [j for j in range(49) if j not in mapped]
    assert len(mapped) == 17 and min(mapped) >= 25 and len([j for j in rest if j >= 25]) == 7
    assert torch.equal(kp[:, mapped], base["smpl_j2d"][:, mapped]) and float(kp[:, rest].abs().sum()) == 0.0
    assert torch.equal(fr["image"], base["image"]) and sorted(fr) == ["bbox", "image", "imgname", "row", "smpl_j2d"]
    for tag in ("full_i2", "full_i2_gated"):
        g, z = golden(f"g10_internet_stream_{tag}.npz"), golden(f"g10_internet_stream_{tag}_noise.npz")
        assert int(g["nframes"]) == 5 and [str(x) for x in g["names"]] == [str(x) for x in z["names"]]
        assert all(f"pred{i}_{k}" in g.files for i in range(5) for k in ("verts", "cam", "rotmat", "beta")) and g["pred0_verts"].shape == (1, 6890, 3)
        assert all(f"frame_{q}_nd_{d}" in z.files for q in "mvdt" for d in ("ref", "or", "o2"))
        assert np.array_equal(g["extra_steps"], z["extra_steps"])
    g = golden("g10_internet_stream_full_i2_gated.npz")
    steps = g["extra_steps"].tolist()
    assert any(1 <= e <= 2 for e in steps) and any(e == 3 for e in steps) and float(g["gate_margin"]) >= 0.02
    assert golden("g10_internet_stream_full_i2.npz")["extra_steps"].tolist() == [0] * 5
