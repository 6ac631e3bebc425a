"""Cases shared by tests/test_crop_many_emu.py (kernel emulator, CPU) and tests/test_crop_many_gpu.py (cuda:0): the many-crop entry
``dyb_crop_resize_normalize_many`` against the single-crop entry ``dyb_crop_resize_normalize`` called for each crop alone - bit for
bit - and ``datasets.preprocess_frames`` against the oracle's crop().  Small on purpose: frames about 64 x 48, res 16 .. 32.

The two entries are driven through the library itself with integer box corners (``datasets.crop_box`` only makes square boxes)."""
import ctypes

import numpy as np
import torch

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -3, -4


def frame(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _ip(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None


def single(lib, img, box, res, out=None):
    """One crop through the single entry.  img: uint8 (H, W, 3) tensor on the device; box = (ul_x, ul_y, br_x, br_y)."""
    dev = img.device
    ws = torch.empty(max(int(lib.dyb_crop_workspace_bytes(box[3] - box[1], box[2] - box[0])), 64), dtype=torch.uint8, device=dev)
    out = torch.full((3, res, res), float("nan"), device=dev) if out is None else out
    rc = lib.dyb_crop_resize_normalize(img.data_ptr(), img.shape[0], img.shape[1], *[int(b) for b in box], out.data_ptr(), res, *MEAN, *STD,
                                       ws.data_ptr(), ws.numel(), _stream(dev))
    assert rc == 0, rc
    return out


def many_raw(lib, imgs, boxes, res, n=None, staging=None):
    """All crops through ONE call of the many entry -> (rc, out [n][3][res][res] pre-filled with NaN).  `n` overrides the count
    that is passed (the error cases)."""
    dev = imgs[0].device
    k = len(imgs)
    n = k if n is None else n
    b = np.asarray(boxes, dtype=np.int32).reshape(k, 4)
    cols = [np.ascontiguousarray(b[:, j]) for j in range(4)]
    bh, bw = cols[3] - cols[1], cols[2] - cols[0]
    H = np.array([im.shape[0] for im in imgs], dtype=np.int32)
    W = np.array([im.shape[1] for im in imgs], dtype=np.int32)
    out = torch.full((k, 3, res, res), float("nan"), device=dev)
    ip = np.array([im.data_ptr() for im in imgs], dtype=np.uint64)
    op = np.array([out[i].data_ptr() for i in range(k)], dtype=np.uint64)
    ws_bytes = int(lib.dyb_crop_many_workspace_bytes(k, _ip(bh), _ip(bw))) if 1 <= k <= 64 else 0
    ws = torch.empty(max(ws_bytes, 1 << 16), dtype=torch.uint8, device=dev)
    if staging is None:
        staging = torch.empty(max(int(lib.dyb_crop_many_staging_bytes(64)), 64), dtype=torch.uint8, pin_memory=dev.type == "cuda")
    rc = lib.dyb_crop_resize_normalize_many(n, _ip(ip), _ip(H), _ip(W), _ip(cols[0]), _ip(cols[1]), _ip(cols[2]), _ip(cols[3]), _ip(op), res,
                                            *MEAN, *STD, staging.data_ptr(), staging.numel(), ws.data_ptr(), ws.numel(), _stream(dev))
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)              # the staging block and the pointer arrays die with this frame
    return rc, out


def assert_many_equals_single(lib, frames, which, boxes, res, device):
    """frames: list of numpy uint8 frames; which[i]: the frame crop i is cut from."""
    dev = torch.device(device)
    on_dev = [torch.from_numpy(f).to(dev) for f in frames]
    imgs = [on_dev[w] for w in which]
    rc, got = many_raw(lib, imgs, boxes, res)
    assert rc == 0, rc
    for i, (im, box) in enumerate(zip(imgs, boxes)):
        want = single(lib, im, box, res)
        assert not torch.isnan(want).any()
        assert torch.equal(got[i], want), (i, box, float((got[i] - want).abs().max()))


F_A, F_B = (48, 64, 1), (37, 53, 2)              # (H, W, seed): two frames of different sizes

# name -> (frame specs, which frame each crop reads, boxes (ul_x, ul_y, br_x, br_y), res)
BOX_CASES = {
    "n1": ([F_A], [0], [(10, 5, 40, 35)], 16),
    "n3_shared_frame_and_other_size": ([F_A, F_B], [0, 0, 1], [(3, 4, 33, 34), (20, 10, 60, 40), (5, 2, 45, 30)], 24),
    "off_left": ([F_A], [0], [(-12, 8, 20, 40)], 16),
    "off_top": ([F_A], [0], [(8, -15, 40, 17)], 16),
    "off_right": ([F_A], [0], [(40, 8, 80, 40)], 16),
    "off_bottom": ([F_A], [0], [(8, 30, 40, 62)], 16),
    "off_all_sides_in_one_call": ([F_A], [0, 0, 0, 0], [(-12, 8, 20, 40), (8, -15, 40, 17), (40, 8, 80, 40), (8, 30, 40, 62)], 16),
    "contains_whole_frame": ([F_A], [0], [(-9, -14, 75, 70)], 32),
    "non_square": ([F_A, F_B], [0, 1], [(4, 6, 61, 25), (10, 1, 22, 36)], 20),
    "upscale_next_to_12x_downscale": ([F_A], [0, 0], [(20, 20, 28, 28), (-60, -70, 132, 122)], 16),    # radius 0 | 192 / 16: radius 22
    "3x3_and_one_pixel_high": ([F_A], [0, 0, 0], [(30, 20, 33, 23), (10, 12, 15, 13), (50, 3, 51, 40)], 16),
}


def n64_case():
    rng = np.random.default_rng(64)
    boxes = []
    for _ in range(64):
        x, y = int(rng.integers(-10, 50)), int(rng.integers(-10, 36))
        boxes.append((x, y, x + int(rng.integers(1, 70)), y + int(rng.integers(1, 70))))
    return [F_A, F_B, (20, 31, 3)], [int(v) for v in rng.integers(0, 3, 64)], boxes, 16


def run_box_case(lib, name, device):
    specs, which, boxes, res = n64_case() if name == "n64" else BOX_CASES[name]
    assert_many_equals_single(lib, [frame(*s) for s in specs], which, boxes, res, device)


def check_error_returns(lib, device):
    """n = 0, n = 65, an empty box, a tap table over CROP_MAX_TAPS (129): the call returns its error before anything is launched -
    outputs pre-filled with NaN stay NaN, those of the valid crops of the same call included."""
    dev = torch.device(device)
    img = torch.from_numpy(frame(*F_A)).to(dev)
    ok = (5, 5, 37, 37)
    for n_pass, k, boxes, want in ((0, 1, [ok], ERR_ARG), (65, 65, [ok] * 65, ERR_ARG),
                                   (2, 2, [ok, (10, 10, 10, 30)], ERR_ARG), (2, 2, [ok, (10, 30, 40, 20)], ERR_ARG),
                                   (2, 2, [ok, (0, 0, 16 * 34, 16)], ERR_UNSUPPORTED)):       # 34x: sigma 16.5, radius 66 -> 133 taps
        rc, out = many_raw(lib, [img] * k, boxes, 16, n=n_pass)
        assert rc == want, (n_pass, boxes[-1], rc)
        assert bool(torch.isnan(out).all()), (n_pass, boxes[-1])
    # a short workspace or staging block is an error as well, not an overrun
    b = np.array([[5, 5, 37, 37]], dtype=np.int32)
    bh = np.array([32], dtype=np.int32)
    assert lib.dyb_crop_many_workspace_bytes(0, _ip(bh), _ip(bh)) == 0 and lib.dyb_crop_many_staging_bytes(65) == 0
    need = int(lib.dyb_crop_many_workspace_bytes(1, _ip(bh), _ip(bh)))
    out = torch.full((1, 3, 16, 16), float("nan"), device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    st = torch.empty(int(lib.dyb_crop_many_staging_bytes(1)), dtype=torch.uint8, pin_memory=dev.type == "cuda")
    ptr = lambda v: _ip(np.array([v], dtype=np.uint64))
    col = lambda j: _ip(np.ascontiguousarray(b[:, j]))
    hh, ww = np.array([48], dtype=np.int32), np.array([64], dtype=np.int32)
    for st_bytes, ws_bytes in ((st.numel(), need - 1), (st.numel() - 1, need)):
        rc = lib.dyb_crop_resize_normalize_many(1, ptr(img.data_ptr()), _ip(hh), _ip(ww), col(0), col(1), col(2), col(3), ptr(out.data_ptr()), 16,
                                                *MEAN, *STD, st.data_ptr(), st_bytes, ws.data_ptr(), ws_bytes, _stream(dev))
        assert rc == ERR_WORKSPACE, rc
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    assert bool(torch.isnan(out).all())


# ---- datasets.preprocess_frames (centre / scale interface) ------------------------------------------------------------------
CS_CASES = [((32.0, 24.0), 0.10, 0), ((50.0, 30.0), 0.22, 0), ((20.0, 18.0), 0.15, 1), ((60.0, 5.0), 0.30, 0), ((26.0, 18.0), 0.40, 1)]


def check_python_entry(device, res=16, reps=1):
    """preprocess_frames == preprocess_frame per crop, bit for bit, and both within the single entry's bound (2e-4 in normalised
    units, tests/test_preprocess.py) of the oracle's crop() + normalisation."""
    from dynaboa_amd import datasets as D
    from oracle import ref_cpu as O
    dev = torch.device(device)
    frames = [frame(*F_A), frame(*F_B)]
    on_dev = [torch.from_numpy(f).to(dev) for f in frames]
    cs = CS_CASES * reps
    out = torch.full((len(cs), 3, res, res), float("nan"), device=dev)
    v0 = out._version
    got = D.preprocess_frames([on_dev[w] for _, _, w in cs], [c for c, _, _ in cs], [s for _, s, _ in cs], res=res, out=out)
    assert got is out and out._version > v0 and tuple(got.shape) == (len(cs), 3, res, res)
    mean, std = np.array(MEAN, np.float32)[:, None, None], np.array(STD, np.float32)[:, None, None]
    for i, (c, s, w) in enumerate(cs[:len(CS_CASES)]):
        assert torch.equal(got[i], D.preprocess_frame(on_dev[w], np.array(c), s, res=res)), i
        want = (np.transpose(O.crop(frames[w].astype(np.float32), np.array(c), s, [res, res]), (2, 0, 1)) / 255.0 - mean) / std
        err = float(np.abs(got[i].cpu().numpy() - want).max())
        print(f"crop {i}: max deviation from the oracle {err:.3e}")
        assert err < 2e-4, (i, err)
    for i in range(len(CS_CASES), len(cs)):                   # the chunks above 64 crops repeat the first ones
        assert torch.equal(got[i], got[i % len(CS_CASES)]), i
    return got
