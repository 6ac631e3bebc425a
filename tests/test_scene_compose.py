"""All tracked people of a video frame in one picture (internet.compose_scenes, --scene_overlays / --compose_only): on a synthetic
folder with hand-written ``Pred_{n}.pt`` files and a small-face renderer on the kernel emulator, and - under `-m gpu` - behind the
driver on cuda:0.  The oracle is the chain  img = frame; for person in order: img = Renderer.render(img, person)  in the documented
order (ascending frame scale sx, then track, then row) and colours (render.track_color); equal bytes."""
import ctypes
import json
import os
import shutil

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from render_cases import icosphere

SEQ = "vid"
W, H = 64, 48
# row -> (frame, track, crop camera (s, tx, ty), box centre, box height); three tracks that start at frames 0, 1 and 2.  In frame 2
# tracks 1 and 2 have the same frame scale (same s, same box height: the tie goes to the lower track id) and track 0, listed first,
# is the largest: painter order there is rows 4, 5, 3.  In frame 1 the order by scale is the reverse of the row order.
ROWS = [(0, 0, (0.9, 0.05, -0.1), (30.0, 22.0), 34.0),
        (1, 0, (0.9, 0.0, 0.1), (30.0, 24.0), 34.0), (1, 1, (0.8, 0.1, 0.0), (40.0, 26.0), 26.0),
        (2, 0, (0.9, -0.1, 0.0), (32.0, 24.0), 34.0), (2, 1, (0.8, 0.0, 0.1), (42.0, 22.0), 26.0), (2, 2, (0.8, 0.1, -0.1), (24.0, 28.0), 26.0)]


@pytest.fixture(scope="module")
def emu_lib():
    from emu.build_emu import build
    from dynaboa_amd import _abi, _lib
    lib = _abi.bind(ctypes.CDLL(build()))
    saved = _lib._lib
    _lib.use_library(lib)
    yield lib
    _lib._lib = saved


def cam_t_of(cam):
    """What the dumps store (benchmark.Adaptor.dump_prediction), in fp32 as there."""
    s, tx, ty = (np.float32(c) for c in cam)
    return np.array([[tx, ty, np.float32(2 * 5000.) / (np.float32(224) * s + np.float32(1e-9))]], np.float32)


@pytest.fixture
def video(tmp_path):
    """-> (root, exppath, faces): <root>/vid.npz, three 64 x 48 frames, <exppath>/result/Pred_{n}.pt with sphere vertices."""
    import joblib
    from PIL import Image
    root, exp = tmp_path / "video", tmp_path / "exp" / "run"
    os.makedirs(root / "images" / SEQ)
    os.makedirs(exp / "result")
    rng = np.random.default_rng(11)
    for f in range(3):
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(root / "images" / SEQ / f"{f:06d}.png")
    np.savez(root / f"{SEQ}.npz", imgname=[os.path.join(SEQ, f"{r[0]:06d}.png") for r in ROWS], center=[r[3] for r in ROWS],
             scale=[r[4] / 200 for r in ROWS], part=np.zeros((len(ROWS), 49, 3)), track=np.array([r[1] for r in ROWS], np.int64))
    v, faces = icosphere(1)
    for n, r in enumerate(ROWS):
        verts = (v * np.float32(1.0 - 0.05 * n)).astype(np.float32)
        verts[:, 2] += 3.0
        joblib.dump({'verts': verts[None], 'cam': cam_t_of(r[2]), 'rotmat': np.zeros((1, 24, 3, 3), np.float32), 'beta': np.zeros((1, 10), np.float32)},
                    exp / "result" / f"Pred_{n}.pt")
    return root, str(exp), faces


def person(ds, exppath, n, width, height):
    """(verts, frame camera fp32, colour) of row n from its dump, by the documented route: parse_cam, then the row's box."""
    import joblib
    from dynaboa_amd.render import convert_crop_cam_to_orig_img, parse_cam, track_color
    d = joblib.load(os.path.join(exppath, "result", f"Pred_{n}.pt"))
    bbox = np.array([[ds.centers[n][0], ds.centers[n][1], ds.scales[n] * 200]], np.float64)
    ocam = convert_crop_cam_to_orig_img(parse_cam(d["cam"].astype(np.float64)), bbox, width, height)[0].astype(np.float32)
    return d["verts"][0], ocam, track_color(int(ds.tracks[n]))


def chain(renderer_of, dev, frame, people):
    r = renderer_of(frame.shape[1], frame.shape[0])
    img = torch.as_tensor(frame).to(dev)
    for v, cam, col in people:
        img = r.render(img, torch.as_tensor(v).to(dev), torch.as_tensor(cam).to(dev), color=col)
    return img.cpu().numpy()


def read_png(path):
    from PIL import Image
    return np.array(Image.open(path).convert("RGB"))


# ---------------------------------------------------------------------------- host and emulator
def test_compose_scenes_equals_the_chain_in_the_documented_order(emu_lib, video):
    from dynaboa_amd import internet as I
    from dynaboa_amd.render import Renderer
    root, exp, faces = video
    ds = I.InternetDataset(None, root=str(root), device="cpu", split_tracks=1)
    assert [(s["track"], s["first"], s["frames"]) for s in ds.sequences] == [(0, 0, 3), (1, 2, 2), (2, 5, 1)]
    paths = I.compose_scenes(ds, exp, renderer=Renderer(faces=faces, device="cpu"))
    assert paths == [os.path.join(exp, "scene", SEQ, f"{f:06d}.png") for f in range(3)]              # one per distinct frame
    assert sorted(os.listdir(os.path.join(exp, "scene", SEQ))) == [f"{f:06d}.png" for f in range(3)]
    renderer_of = lambda w, h: Renderer(resolution=(w, h), faces=faces, device="cpu")
    order = {0: [0], 1: [2, 1], 2: [4, 5, 3]}                   # ascending sx = s * box height / W, then track
    for f in range(3):
        frame = ds.read_frame(os.path.join(SEQ, f"{f:06d}.png"))
        people = [person(ds, exp, n, W, H) for n in order[f]]
        assert [p[1][0] for p in people] == sorted(p[1][0] for p in people)
        want = chain(renderer_of, "cpu", frame, people)
        got = read_png(paths[f])
        assert got.shape == (H, W, 3) and got.tobytes() == want.tobytes(), f
        assert (want != frame).any(-1).sum() > 100
        if len(people) > 1:                                     # the order matters: the reverse chain is another picture
            assert chain(renderer_of, "cpu", frame, people[::-1]).tobytes() != want.tobytes()
    # frame 0 has one person: the scene is that row's single overlay
    v, cam, col = person(ds, exp, 0, W, H)
    single = renderer_of(W, H).render(ds.read_frame(os.path.join(SEQ, "000000.png")), v, cam, color=col)
    assert read_png(paths[0]).tobytes() == np.asarray(single).tobytes()
    assert col == tuple(c / 255.0 for c in (205, 129, 98))
    # rows: only those people are drawn
    only = I.compose_scenes(ds, exp, renderer=Renderer(faces=faces, device="cpu"), rows=[3, 5])
    assert only == [paths[2]]
    frame = ds.read_frame(os.path.join(SEQ, "000002.png"))
    assert read_png(paths[2]).tobytes() == chain(renderer_of, "cpu", frame, [person(ds, exp, 5, W, H), person(ds, exp, 3, W, H)]).tobytes()


def test_missing_dump_names_the_row(emu_lib, video):
    from dynaboa_amd import internet as I
    from dynaboa_amd.render import Renderer
    root, exp, faces = video
    os.remove(os.path.join(exp, "result", "Pred_4.pt"))
    ds = I.InternetDataset(None, root=str(root), device="cpu")
    with pytest.raises(FileNotFoundError, match=r"row 4 .*Pred_4\.pt"):
        I.compose_scenes(ds, exp, renderer=Renderer(faces=faces, device="cpu"))


def test_parse_cam_inverts_the_dumped_camera():
    from dynaboa_amd.render import parse_cam
    for s in np.linspace(0.3, 3.0, 28):
        ct = cam_t_of((s, 0.25, -0.5))
        for got in (parse_cam(ct), parse_cam(torch.from_numpy(ct)).numpy(), parse_cam(ct.astype(np.float64))):
            assert got.shape == (1, 3) and abs(float(got[0, 0]) - s) <= 1e-6 * s, (s, got)
            assert float(got[0, 1]) == 0.25 and float(got[0, 2]) == -0.5
    assert torch.is_tensor(parse_cam(torch.from_numpy(cam_t_of((1.0, 0.0, 0.0)))))


def test_track_colours():
    from dynaboa_amd import constants as C
    from dynaboa_amd.render import track_color
    ref = (205 / 255.0, 129 / 255.0, 98 / 255.0)
    assert track_color(-1) == track_color(0) == ref
    n = len(C.TRACK_COLORS)
    assert n >= 8 and len(set(C.TRACK_COLORS)) == n and all(len(c) == 3 and all(0 <= x <= 255 for x in c) for c in C.TRACK_COLORS)
    assert [track_color(t) for t in range(n)] == [tuple(x / 255.0 for x in c) for c in C.TRACK_COLORS]
    assert track_color(n) == track_color(0) and track_color(2 * n + 3) == track_color(3)


def test_scene_overlays_with_shards_are_refused_before_any_adaptation(video, tmp_path, monkeypatch):
    from dynaboa_amd import internet as I
    root, _, _ = video
    monkeypatch.setattr(I, "Adaptor", lambda *a, **k: pytest.fail("an adaptor was built"))
    monkeypatch.setattr(I, "InternetDataset", lambda *a, **k: pytest.fail("the dataset was read"))
    for flag in ("--scene_overlays", "--compose_only"):
        o = I.parser.parse_args(["--internet_root", str(root), "--expdir", str(tmp_path / "none"), "--expname", "run", "--split_tracks", "1",
                                 "--num_shards", "2", flag, "1"])
        with pytest.raises(ValueError, match=r"--compose_only 1"):
            I.run_driver(o, device=torch.device("cpu"))
    assert not os.path.exists(tmp_path / "none")
    o = I.parser.parse_args([])
    assert (o.scene_overlays, o.compose_only) == (0, 0)


# ---------------------------------------------------------------------------- the driver on the GPU
SHORT = ["--inner_step", "1", "--interval", "2", "--optim_steps", "2"]


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """The g10 detections of the first five frames (track 0: 5 rows, track 1: 4 - its frame 3 fails the score test) over 1280 x 720
    frames."""
    from PIL import Image
    from dynaboa_amd import internet as I
    root = tmp_path_factory.mktemp("video")
    with open(os.path.join(GOLDEN, "g10_internet_detections.json")) as fh:
        dets = [d for d in json.load(fh) if d["image_id"] in [f"{f:06d}.png" for f in range(5)]]
    with open(root / "g10seq.json", "w") as fh:
        json.dump(dets, fh)
    os.makedirs(root / "images" / "g10seq")
    yy, xx = np.mgrid[0:720, 0:1280]
    for f in range(5):
        img = np.stack([(xx // 5 + 9 * f) % 256, (yy // 3 + 5 * f) % 256, ((xx + yy) // 7 + 3 * f) % 256], -1).astype(np.uint8)
        Image.fromarray(img).save(root / "images" / "g10seq" / f"{f:06d}.png")
    I.main(["--extract", str(root)])
    return root


def _drive(folder, exp, *flags):
    from dynaboa_amd import internet as I
    from dynaboa_amd.base_adaptor import synthetic_bundle
    bundle = synthetic_bundle(seed=22, identity_pose=False, randomize_norm=True, smpl_seed=0)
    o = I.parser.parse_args(["--internet_root", str(folder), "--expdir", str(exp), "--expname", "run", *SHORT, *flags])
    res = I.run_driver(o, assets_bundle=bundle, device=torch.device("cuda:0"))
    torch.cuda.synchronize()
    return res, os.path.join(str(exp), "run"), bundle


@pytest.mark.gpu
def test_driver_scene_overlays_gpu(folder, tmp_path):
    from dynaboa_amd import internet as I, native_step as NS
    from dynaboa_amd.render import Renderer
    try:
        rows, run, bundle = _drive(folder, tmp_path, "--split_tracks", "1", "--seqs_per_gpu", "2", "--scene_overlays", "1")
    finally:
        NS.set_replica_policy(False)
    assert sorted(rows) == list(range(9))
    names = [f"{f:06d}.png" for f in range(5)]
    assert sorted(os.listdir(os.path.join(run, "scene", "g10seq"))) == names
    dev = "cuda:0"
    ds = I.InternetDataset(None, root=str(folder), device=dev, split_tracks=1)
    faces = np.asarray(bundle.smpl_neutral["faces"])
    renderer_of = lambda w, h: Renderer(resolution=(w, h), faces=faces, device=dev)
    first = {}
    for f, name in enumerate(names):
        here = [n for n in range(len(ds)) if str(ds.imgnames[n]) == os.path.join("g10seq", name)]
        assert len(here) == (1 if f == 3 else 2)
        people = sorted((person(ds, run, n, 1280, 720) + (int(ds.tracks[n]), n) for n in here), key=lambda p: (p[1][0], p[3], p[4]))
        frame = ds.read_frame(os.path.join("g10seq", name))
        want = chain(renderer_of, dev, frame, [p[:3] for p in people])
        first[name] = open(os.path.join(run, "scene", "g10seq", name), "rb").read()
        got = read_png(os.path.join(run, "scene", "g10seq", name))
        assert got.shape == (720, 1280, 3) and got.tobytes() == want.tobytes(), name
        assert (want != frame).any(-1).sum() > 1000
    # --compose_only 1 over the same directory: the same files again
    shutil.rmtree(os.path.join(run, "scene"))
    paths, _, _ = _drive(folder, tmp_path, "--split_tracks", "1", "--compose_only", "1")
    assert sorted(paths) == [os.path.join(run, "scene", "g10seq", n) for n in names]
    assert all(open(p, "rb").read() == first[os.path.basename(p)] for p in paths)


@pytest.mark.gpu
def test_driver_without_the_flags_writes_no_scene_directory_gpu(folder, tmp_path):
    rows, run, _ = _drive(folder, tmp_path, "--split_tracks", "1", "--min_track_frames", "5")
    assert len(rows) == 5 and len(os.listdir(os.path.join(run, "result"))) == 5
    assert not os.path.exists(os.path.join(run, "scene"))
