"""The device JPEG encoder behind the drivers, on cuda:0: JpegEncoder on the rasteriser's pictures against PIL's own encoding of the
same pixels, the retry of a picture that did not fit, and --overlay_format jpg / --overlay_video 1 on the synthetic bundle (3 frames,
224 x 224 crops) - the .jpg files hold the scans PIL gives for what the same run writes as .png, the .avi files hold those files in
order, one per sequence, and a run without the new flags writes what it always wrote."""
import io
import os
import struct

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

FRAME_ONLY = dict(retrieval=0, lower_level_mixtrain=0, upper_level_mixtrain=0, use_meanteacher=0, use_motion=0,
                  dynamic_boa=0, use_temporal_losses_upper=0, inner_step=1)
NF = 3


def _mk(r, opts, expdir):
    from dynaboa_amd import benchmark as DB
    from dynaboa_amd.base_adaptor import synthetic_bundle
    o = DB.parser.parse_args([])
    for k, v in {**FRAME_ONLY, "deferred_metrics": 0, **opts}.items():
        setattr(o, k, v)
    o.expdir, o.expname = str(expdir), "jp"
    return DB.Adaptor(o, synthetic_bundle(seed=22 + r, identity_pose=False, randomize_norm=True, smpl_seed=0), device="cuda:0")


def _frames(S):
    from dynaboa_amd import assets
    return [[{k: v.to("cuda:0") for k, v in assets.make_frame(100 * r + s, 1, seed=22).items()} for s in range(NF)] for r in range(S)]


def _pil_jpeg(rgb, quality, subsampling):
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", quality=quality, subsampling=0 if subsampling == 444 else 2)
    return buf.getvalue()


def _scan(data):
    i = 2
    while data[i + 1] != 0xDA:
        i += 2 + int.from_bytes(data[i + 2:i + 4], "big")
    i += 2 + int.from_bytes(data[i + 2:i + 4], "big")
    assert data[-2:] == b"\xff\xd9"
    return data[i:-2]


def _avi_frames(path):
    """the payloads of the 00dc chunks of LIST movi, in file order"""
    data = open(path, "rb").read()
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI " and struct.unpack("<I", data[4:8])[0] == len(data) - 8
    at, out = 12, []
    while at < len(data):
        cc, n = data[at:at + 4], struct.unpack("<I", data[at + 4:at + 8])[0]
        if cc == b"LIST" and data[at + 8:at + 12] == b"movi":
            k, end = at + 12, at + 8 + n
            while k < end:
                assert data[k:k + 4] == b"00dc"
                m = struct.unpack("<I", data[k + 4:k + 8])[0]
                out.append(data[k + 8:k + 8 + m])
                k += 8 + m + (m & 1)
        at += 8 + n + (n & 1)
    return out


def _same_as_pil(files, pics, quality, subsampling):
    for data, pic in zip(files, pics):
        rgb = pic.cpu().numpy()
        theirs = _pil_jpeg(rgb, quality, subsampling)
        assert _scan(data) == _scan(theirs)
        im = Image.open(io.BytesIO(data))
        assert im.size == (rgb.shape[1], rgb.shape[0]) and im.mode == "RGB"
        assert np.array_equal(np.asarray(im), np.asarray(Image.open(io.BytesIO(theirs))))


@pytest.mark.parametrize("subsampling", [444, 420])
def test_encoder_on_rendered_pictures_equals_pil(subsampling, tmp_path):
    from dynaboa_amd.base_adaptor import synthetic_bundle
    from dynaboa_amd.jpeg import JpegEncoder
    from dynaboa_amd.render import Renderer
    from dynaboa_amd.smpl import SMPL
    dev = torch.device("cuda:0")
    smpl = SMPL(tables=synthetic_bundle(seed=22, smpl_seed=0).smpl_neutral).to(dev)
    with torch.no_grad():
        vts = smpl(betas=torch.zeros(2, 10, device=dev), body_pose=torch.zeros(2, 69, device=dev),
                   global_orient=torch.zeros(2, 3, device=dev)).vertices
    rng = np.random.default_rng(3)
    frames = [torch.from_numpy(rng.integers(0, 256, s, dtype=np.uint8)).to(dev) for s in ((128, 256, 3), (144, 72, 3))]
    cams = torch.tensor([[0.75, 1.5, 0.0, 0.0], [1.0, 0.5, 0.0, 0.1]], device=dev)
    pics = Renderer(faces=smpl.faces, device=dev).render_many(frames, [vts[0], vts[1]], cams)
    assert any((p != f).any() for p, f in zip(pics, frames))        # meshes are on the frames
    enc = JpegEncoder(dev, quality=90, subsampling=subsampling)
    files = enc.encode(pics)
    _same_as_pil(files, pics, 90, subsampling)
    assert enc.retries == 0 and enc.bytes_to_host == sum(len(_scan(f)) for f in files) + 16
    assert files == enc.encode(pics)                                 # the kept buffers: a second call returns the same files
    paths = enc.save(pics, [str(tmp_path / "a.jpg"), str(tmp_path / "b.jpg")])
    assert [open(p, "rb").read() for p in paths] == files


def test_encoder_retries_a_picture_that_did_not_fit():
    from dynaboa_amd.jpeg import JpegEncoder
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(5)
    noise = torch.from_numpy(rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)).to(dev)
    calm = torch.full((40, 56, 3), 77, dtype=torch.uint8, device=dev)
    enc = JpegEncoder(dev, quality=100, subsampling=444)
    files = enc.encode([calm, noise, calm])
    assert len(_scan(files[1])) > 48 * 64 * 3 // 2 + 4096 and enc.retries == 1        # more than its room, indeed more than raw
    _same_as_pil(files, [calm, noise, calm], 100, 444)


def _run_single(root, **opts):
    ad = _mk(0, dict(save_res=1, **opts), root)
    ad.excute(_frames(1)[0], nframes=NF)
    torch.cuda.synchronize()
    return ad


def test_driver_writes_jpg_and_video(tmp_path):
    """the autograd path of --save_res 1 (what tests/test_save_res_gpu.py pins for PNG)"""
    _run_single(tmp_path / "png")
    image = tmp_path / "png" / "jp" / "image"
    names = [f"Pred_{i}.png" for i in range(NF)]
    assert sorted(os.listdir(image)) == names and sorted(os.listdir(tmp_path / "png" / "jp")) == ["image"]      # no video/
    ad = _run_single(tmp_path / "jpg", overlay_format="jpg", overlay_video=1, video_fps=25.0)
    out = tmp_path / "jpg" / "jp"
    assert sorted(os.listdir(out / "image")) == [f"Pred_{i}.jpg" for i in range(NF)]
    files = [open(out / "image" / f"Pred_{i}.jpg", "rb").read() for i in range(NF)]
    for i, data in enumerate(files):
        want = np.array(Image.open(image / names[i]))
        assert want.shape == (224, 224, 3)
        assert _scan(data) == _scan(_pil_jpeg(want, 90, 444))
    assert os.listdir(out / "video") == ["Pred_sequence.avi"]
    assert _avi_frames(out / "video" / "Pred_sequence.avi") == files
    assert ad.overlay_sink() is not None and not ad.overlay_sink()._writers       # excute closed the video

    # the video alone: PNG files as ever, the video beside them, 4:2:0 at quality 60
    _run_single(tmp_path / "vid", overlay_video=1, jpeg_quality=60, jpeg_subsampling="420")
    out = tmp_path / "vid" / "jp"
    assert sorted(os.listdir(out / "image")) == names
    frames = _avi_frames(out / "video" / "Pred_sequence.avi")
    assert len(frames) == NF
    for i, data in enumerate(frames):
        assert open(out / "image" / names[i], "rb").read() == open(image / names[i], "rb").read()
        assert _scan(data) == _scan(_pil_jpeg(np.array(Image.open(image / names[i])), 60, 420))


def test_online_driver_writes_jpg_and_pred_avi(tmp_path):
    """python -m dynaboa_amd.online on three frames: Pred_{n}.png as ever without the flags, Pred_{n}.jpg and Pred.avi with them"""
    from dynaboa_amd import online as ON
    from dynaboa_amd.base_adaptor import synthetic_bundle
    rng = np.random.default_rng(5)
    fdir = tmp_path / "frames"
    fdir.mkdir()
    names, kps = [], []
    for i in range(3):
        Image.fromarray(rng.integers(0, 255, (120, 160, 3), dtype=np.uint8)).save(fdir / f"{i:03d}.png")
        names.append(f"{i:03d}.png")
        kps.append(np.concatenate([rng.uniform(30, 110, (25, 2)), rng.uniform(0.2, 1.0, (25, 1))], 1).astype(np.float32))
    np.savez(tmp_path / "det.npz", imgname=np.array(names), keypoints=np.stack(kps))
    bundle = lambda: synthetic_bundle(seed=22, identity_pose=False, randomize_norm=True, smpl_seed=0)
    base = dict(use_boa=1, interval=2, save_video=1, frames=str(fdir), detections=str(tmp_path / "det.npz"), log_frames=4)
    ON.run_driver(ON.online_options(out=str(tmp_path / "png"), **base), assets_bundle=bundle(), device="cuda:0")
    assert sorted(n for n in os.listdir(tmp_path / "png") if not n.endswith(".npz")) == [f"Pred_{i}.png" for i in range(3)]
    ON.run_driver(ON.online_options(out=str(tmp_path / "jpg"), overlay_format="jpg", overlay_video=1, **base), assets_bundle=bundle(),
                  device="cuda:0")
    assert sorted(n for n in os.listdir(tmp_path / "jpg") if not n.endswith(".npz")) == ["Pred.avi"] + [f"Pred_{i}.jpg" for i in range(3)]
    files = [open(tmp_path / "jpg" / f"Pred_{i}.jpg", "rb").read() for i in range(3)]
    for i, data in enumerate(files):
        want = np.array(Image.open(tmp_path / "png" / f"Pred_{i}.png"))
        assert want.shape == (120, 160, 3) and _scan(data) == _scan(_pil_jpeg(want, 90, 444))
    assert _avi_frames(tmp_path / "jpg" / "Pred.avi") == files


def _run_group(root, **opts):
    from dynaboa_amd import native_step as NS
    from dynaboa_amd.base_adaptor import close_overlays
    S = 2
    frames = _frames(S)
    ads = [_mk(r, dict(save_res=1, native_results=1, deferred_metrics=1, side_view=90.0, **opts), root) for r in range(S)]
    for r, a in enumerate(ads):
        a.sequence_name = f"seq{r}"                                  # as the sharded driver names its adaptors
    grp = NS.ReplicaGroup(ads, NF)
    calls = []
    sink = ads[0].overlay_sink()
    if sink is not None:
        inner = sink.encoder.encode
        sink.encoder.encode = lambda pics: (calls.append(len(pics)), inner(pics))[1]
    try:
        for s in range(NF):
            grp.step([frames[r][s] for r in range(S)], s, result_steps=[10 * r + s for r in range(S)])
        grp.stepper.join()
        torch.cuda.synchronize()
    finally:
        if sink is not None:
            sink.encoder.encode = inner
        close_overlays(ads)
    assert sink is None or not sink._writers
    return calls


def test_group_with_side_views_writes_jpg_and_one_video_per_sequence(tmp_path):
    """--native_results 1 with two sequences in lockstep and --side_view 90: panels of twice the width, joined on the device"""
    assert _run_group(tmp_path / "png") == []
    image = tmp_path / "png" / "jp" / "image"
    numbers = [10 * r + s for r in range(2) for s in range(NF)]
    assert sorted(os.listdir(image)) == sorted(f"Pred_{n}.png" for n in numbers)
    assert sorted(os.listdir(tmp_path / "png" / "jp")) == ["image"]
    calls = _run_group(tmp_path / "jpg", overlay_format="jpg", overlay_video=1)
    assert calls == [2] * NF                                         # both sequences' panels of a step in ONE encode call
    out = tmp_path / "jpg" / "jp"
    assert sorted(os.listdir(out / "image")) == sorted(f"Pred_{n}.jpg" for n in numbers)
    files = {}
    for n in numbers:
        want = np.array(Image.open(image / f"Pred_{n}.png"))
        assert want.shape == (224, 448, 3)
        files[n] = open(out / "image" / f"Pred_{n}.jpg", "rb").read()
        assert _scan(files[n]) == _scan(_pil_jpeg(want, 90, 444))
    assert sorted(os.listdir(out / "video")) == ["Pred_seq0.avi", "Pred_seq1.avi"]
    for r in range(2):
        assert _avi_frames(out / "video" / f"Pred_seq{r}.avi") == [files[10 * r + s] for s in range(NF)]


def test_sharded_driver_writes_one_video_per_sequence_and_closes_them(tmp_path):
    """run_sharded with two sequences per GPU over three sequences of 3, 2 and 2 frames - a lockstep wave of two (the shorter one
    leaves the launch set) and a wave of one, which goes through excute - all adaptors writing into ONE exppath.  The driver's own
    options carry no overlay flag (the adaptors' do, as in tests/test_native_results_gpu.py); a sequence is named by a file path,
    as 3DPW's are.  One video/Pred_{sequence name}.avi per sequence with that sequence's .jpg files in order, and every writer
    closed when run_sharded returns."""
    from dynaboa_amd import benchmark as DB
    from dynaboa_amd.sharded import SequenceSpec, run_sharded
    lens = [3, 2, 2]
    frames = _frames(len(lens))
    specs, first = [], 0
    for k, n in enumerate(lens):
        specs.append(SequenceSpec(f"extras/3dpw_walk_{k}.npz", first, n, (lambda k=k, n=n: frames[k][:n])))
        first += n
    made = []

    def make():
        made.append(_mk(0, dict(vars(DB.frame_only_options(inner_step=1)), deferred_metrics=1, save_res=1, native_results=1,
                                overlay_format="jpg", overlay_video=1), tmp_path))
        return made[-1]
    res = run_sharded(DB.frame_only_options(inner_step=1), specs, make, num_shards=1, shard_rank=0, seqs_per_gpu=2)
    assert sorted(int(g) for g in res["global_index"]) == list(range(sum(lens))) and len(made) == 3
    sinks = [a.__dict__.get("_overlay_sink") for a in made]
    assert sinks[0] is not None and sinks[2] is not None              # the group's (its first adaptor's) and the lone sequence's
    assert all(s is None or not s._writers for s in sinks)           # nothing is left open
    out = tmp_path / "jp"
    assert sorted(os.listdir(out / "image")) == sorted(f"Pred_{i}.jpg" for i in range(sum(lens)))
    assert sorted(os.listdir(out / "video")) == [f"Pred_3dpw_walk_{k}.avi" for k in range(3)]
    first = 0
    for k, n in enumerate(lens):
        files = [open(out / "image" / f"Pred_{first + i}.jpg", "rb").read() for i in range(n)]
        assert len(set(files)) == n
        assert _avi_frames(out / "video" / f"Pred_3dpw_walk_{k}.avi") == files, k       # (a file never closed has no sizes: refused there)
        first += n
