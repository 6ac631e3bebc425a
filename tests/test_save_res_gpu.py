"""--save_res 1 end to end on cuda:0: an adaptor on the synthetic bundle (built as tests/test_adaptation_gpu.py builds its own)
adapts two frames and leaves one rendered overlay per frame; drawing them changes nothing in the adaptation.

`save_res` routes the run off the native stepper (native_step.coverage: "rendered results", as prediction dumps do), so "the same run
with save_res=0" is the same schedule - the autograd path, native_step=0 - with the flag off; the two are compared bit for bit."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FRAME_ONLY = dict(retrieval=0, lower_level_mixtrain=0, upper_level_mixtrain=0, use_meanteacher=0, use_motion=0,
                  dynamic_boa=0, use_temporal_losses_upper=0, inner_step=1)


def make_adaptor(expdir, **over):
    from dynaboa_amd import benchmark as DB
    from dynaboa_amd.base_adaptor import synthetic_bundle
    o = DB.parser.parse_args([])
    for k, v in dict(FRAME_ONLY, deferred_metrics=0, expdir=str(expdir), expname="save_res", **over).items():
        setattr(o, k, v)
    return DB.Adaptor(o, synthetic_bundle(seed=22, identity_pose=False, randomize_norm=True, smpl_seed=0), device="cuda:0")


def run(ad, nframes=2):
    from dynaboa_amd import assets
    ad.reset_records(nframes)
    metrics, batches = [], []
    for step in range(nframes):
        ad.global_step = step
        ad.fit_losses = {}
        batch = {k: v.to(ad.device) for k, v in assets.make_frame(step, 1, seed=22).items()}
        ad.model.eval()
        metrics.append(ad.adaptation(batch))
        batches.append(batch)
    torch.cuda.synchronize()
    return metrics, batches


def test_coverage_routes_save_res_off_the_stepper():
    from dynaboa_amd import benchmark as DB, native_step as NS
    o = DB.parser.parse_args([])
    for k, v in FRAME_ONLY.items():
        setattr(o, k, v)
    before = NS.coverage(o)
    assert before == ("frame", None)
    o.save_res = 1
    assert NS.coverage(o) == ("", "rendered results")
    o.save_res = 0
    assert NS.coverage(o) == before
    full = DB.parser.parse_args([])
    assert NS.coverage(full)[0] == "full"
    full.save_res = 1
    assert NS.coverage(full) == ("", "rendered results")


def test_save_res_writes_overlays_and_leaves_adaptation_alone(tmp_path):
    from PIL import Image
    from dynaboa_amd import constants as C
    from dynaboa_amd.render import Renderer
    ad = make_adaptor(tmp_path / "on", save_res=1)

    # the picture of a frame is written by the LAST inference() of its adaptation(): record what that call drew from
    seen = {}
    inner = ad.save_results

    def spy(vts, cam, images, name, bbox, prefix=None):
        seen[ad.global_step] = (vts.detach().clone(), cam.detach().clone(), images.detach().clone())
        return inner(vts, cam, images, name, bbox, prefix=prefix)
    ad.save_results = spy
    m_on, _ = run(ad)
    assert ad._native is None and not ad._native_ok()
    files = sorted(os.listdir(tmp_path / "on" / "save_res" / "image"))
    assert files == ["Pred_0.png", "Pred_1.png"]
    r = Renderer(resolution=(224, 224), faces=ad.smpl_neutral.faces)
    mean = torch.tensor(C.IMG_NORM_MEAN, device=ad.device).view(1, 3, 1, 1)
    std = torch.tensor(C.IMG_NORM_STD, device=ad.device).view(1, 3, 1, 1)
    for step in range(2):
        vts, cam, images = seen[step]
        crop = ((images * std + mean) * 255.0).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        ccam = torch.stack([cam[:, 0], cam[:, 0], cam[:, 1], cam[:, 2]], 1)
        want = r.render(crop, vts, ccam, color=(205 / 255.0, 129 / 255.0, 98 / 255.0))[0].cpu().numpy()
        got = np.array(Image.open(tmp_path / "on" / "save_res" / "image" / f"Pred_{step}.png"))
        assert got.shape == (224, 224, 3) and np.array_equal(got, want)
        assert (want != crop[0].cpu().numpy()).any()                 # a mesh is on the crop

    off = make_adaptor(tmp_path / "off", save_res=0, native_step=0)
    m_off, _ = run(off)
    assert not os.path.exists(tmp_path / "off" / "save_res" / "image")
    assert torch.equal(ad.model.module.theta.detach(), off.model.module.theta.detach())
    st_on, st_off = ad.optimizer.state[ad.model.module.theta], off.optimizer.state[off.model.module.theta]
    assert torch.equal(st_on["exp_avg"], st_off["exp_avg"]) and torch.equal(st_on["exp_avg_sq"], st_off["exp_avg_sq"])
    for a, b in zip(m_on, m_off):
        for x, y in zip(a, b):
            assert np.array_equal(np.asarray(x), np.asarray(y))


def test_save_results_over_the_original_frames(tmp_path):
    """The branch real 3DPW streams take: the frames are files under ``imgdir``, the crop camera is converted to each frame with its
    box, and the mesh is drawn at the frame's own size (256 x 128 and 72 x 144: width and height differ, one width is no multiple
    of 16).  The expected camera is worked out here - scale = s h / (W, H), shift = t + (2 c / (W, H) - 1) / scale - from
    numbers for which every step is exact in fp32, so the file must equal the rendering byte for byte."""
    from PIL import Image
    from dynaboa_amd.render import Renderer
    ad = make_adaptor(tmp_path / "exp", save_res=1)
    rng = np.random.default_rng(4)
    frames = [rng.integers(0, 256, (128, 256, 3), dtype=np.uint8), rng.integers(0, 256, (144, 72, 3), dtype=np.uint8)]
    names = ["seq_a/image_00007.png", "seq_b/image_00001.png"]
    for n, f in zip(names, frames):
        os.makedirs(os.path.dirname(tmp_path / "frames" / n), exist_ok=True)
        Image.fromarray(f).save(tmp_path / "frames" / n)
    ad.imgdir = str(tmp_path / "frames")
    ad.global_step = 5
    with torch.no_grad():
        betas = torch.tensor([[0.5] * 10, [-0.5] * 10], device=ad.device)
        pose = torch.zeros(2, 72, device=ad.device)
        vts = ad.smpl_neutral(betas=betas, body_pose=pose[:, 3:], global_orient=pose[:, :3]).vertices
    cam = torch.tensor([[1.5, 0.0, 0.25], [2.0, -0.125, 0.0]], device=ad.device)
    bbox = torch.tensor([[152.0, 52.0, 128.0], [40.5, 81.0, 36.0]], dtype=torch.float64, device=ad.device)       # as PW3D yields it
    #   frame 0: scale = 1.5 * 128 / (256, 128) = (0.75, 1.5), shift = (0 + 0.1875 / 0.75, 0.25 - 0.1875 / 1.5) = (0.25, 0.125)
    #   frame 1: scale = 2 * 36 / (72, 144) = (1, 0.5),       shift = (-0.125 + 0.125 / 1, 0 + 0.125 / 0.5)    = (0, 0.25)
    want_cams = [[0.75, 1.5, 0.25, 0.125], [1.0, 0.5, 0.0, 0.25]]
    paths = ad.save_results(vts, cam, None, names, bbox, prefix="Pred")
    assert [os.path.relpath(p, tmp_path / "exp" / "save_res" / "image") for p in paths] == ["Pred_5.png", "Pred_6.png"]
    for k, frame in enumerate(frames):
        H, W = frame.shape[:2]
        want = Renderer(resolution=(W, H), faces=ad.smpl_neutral.faces).render(
            torch.from_numpy(frame).to(ad.device), vts[k], torch.tensor(want_cams[k], device=ad.device),
            color=(205 / 255.0, 129 / 255.0, 98 / 255.0)).cpu().numpy()
        got = np.array(Image.open(paths[k]))
        drawn = (want != frame).any(-1)
        assert 200 < drawn.sum() < 0.9 * H * W                       # the mesh is on the frame and the frame shows around it
        assert got.shape == frame.shape and np.array_equal(got, want)
