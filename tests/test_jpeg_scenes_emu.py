"""internet.compose_scenes through the JPEG sink (--overlay_format jpg / --overlay_video 1), on the synthetic folder and the kernel
emulator of tests/test_scene_compose.py: the .jpg files hold the scans PIL gives for the pictures the plain pass writes as .png, the
video holds those files in frame order, and JpegEncoder itself runs on host buffers against the emulator library."""
import io
import os

import numpy as np
import torch
from PIL import Image

import jpeg_cases as J
from test_scene_compose import H, SEQ, W, emu_lib, video          # noqa: F401  (fixtures)
from test_jpeg_host import check_avi


def test_encoder_on_the_emulator_equals_the_restatement(emu_lib):
    from dynaboa_amd.jpeg import EOI, JpegEncoder, jpeg_header
    pics = [J.picture(c, h, w) for c, h, w in J.RAGGED]
    for sub in J.SUBSAMPLINGS:
        enc = JpegEncoder("cpu", quality=90, subsampling=sub)
        files = enc.encode([torch.from_numpy(p) for p in pics])
        for (c, h, w), data in zip(J.RAGGED, files):
            assert data == jpeg_header(w, h, 90, sub) + J.want(c, h, w, 90, sub) + EOI
    # too little room by default: noise at quality 100 is encoded again with what its length asks for
    enc = JpegEncoder("cpu", quality=100, subsampling=444)
    noise = J.picture("noise", 48, 64)
    data = enc.encode([torch.from_numpy(noise)])[0]
    assert enc.retries == 1 and len(data) > 48 * 64 * 3 // 2 + 4096
    assert data == jpeg_header(64, 48, 100, 444) + J.scan(noise, 100, 444) + EOI


def test_compose_scenes_writes_jpg_and_a_video(emu_lib, video):
    from dynaboa_amd import internet as I
    from dynaboa_amd.jpeg import OverlaySink
    from dynaboa_amd.render import Renderer
    root, exp, faces = video
    ds = I.InternetDataset(None, root=str(root), device="cpu", split_tracks=1)
    plain = I.compose_scenes(ds, exp, renderer=Renderer(faces=faces, device="cpu"))
    assert sorted(os.listdir(os.path.join(exp, "scene"))) == [SEQ]                       # no video without the flag
    sink = OverlaySink("cpu", "jpg", quality=75, subsampling="420", video=True, fps=24)
    calls = []
    inner = sink.encoder.encode
    sink.encoder.encode = lambda pics: (calls.append(len(pics)), inner(pics))[1]
    paths = I.compose_scenes(ds, exp, renderer=Renderer(faces=faces, device="cpu"), out_dir="scene_jpg", sink=sink)
    assert calls == [3]                                                                  # the pictures of a scene call: ONE encode
    assert paths == [os.path.join(exp, "scene_jpg", SEQ, f"{f:06d}.jpg") for f in range(3)]
    assert sorted(os.listdir(os.path.join(exp, "scene_jpg"))) == [SEQ, SEQ + ".avi"]
    files = []
    for png, jpg in zip(plain, paths):
        want = np.array(Image.open(png).convert("RGB"))
        data = open(jpg, "rb").read()
        assert J.pil_scan(want, 75, 420)[0] in data and data.endswith(J.pil_scan(want, 75, 420)[0] + b"\xff\xd9")
        assert Image.open(io.BytesIO(data)).size == (W, H)
        files.append(data)
    check_avi(os.path.join(exp, "scene_jpg", SEQ + ".avi"), files, W, H, 24, 1)
    assert not sink._writers                                                             # the pass closed its video
