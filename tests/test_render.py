"""The mesh overlay (csrc/render.hip, dynaboa_amd/render.py) against known answers and against tests/render_ref.py, the numpy
restatement of its rules - on the kernel emulator here, on cuda:0 under `-m gpu`.

What is pinned: coverage (exact, integer), the winner per pixel, depth, the smooth shading as this project defines it.  What is NOT:
pyrender's metallic-roughness shading (unpinned: pyrender is absent from the build image); geometry, visibility and the light set-up
are the reference's (render_demo.py:58-134).

Pixels where the kernel (fp32 depth) may name another face than the float64 reference - the kernel's face must cover the pixel by
the integer test and lie within 1e-6 max|Z| of the winner - are capped at 0.1 % of the covered pixels.  Counted on the CPU
(emulator) for every mesh used here: icosphere 80 / 320 faces at 64x64, 70x45 and the three-camera batches: 0 of 431 ... 2023
covered pixels; synthetic SMPL at 224x224, two poses: first 2000 faces 0 of 9785 / 7329, all 13 776 faces 0 of 12 862 / 8926 ; on
an MI355X the same counts, and 0 of 155 856 for the 1920x1080 case, which exists there only (every case prints its count, `-s`)."""
import numpy as np
import pytest
import torch

import render_ref as RR
from render_cases import ZOFF, dev, emu_lib, icosphere, rasterize, smpl_case, sphere_case      # noqa: F401 (fixtures)

# ---------------------------------------------------------------------------- helpers
UNIT16 = (1.0, 1.0, 0.0, 0.0)          # on a 16 x 16 image: u = 8 (1 + X), exact for the coordinates used below


def at(u, v, z=0.0):
    """Model-space vertex that lands on image position (u, v) of a 16 x 16 image under UNIT16 (exact in fp32)."""
    return [u / 8.0 - 1.0, v / 8.0 - 1.0, z]


def right_tri(x0, y0, L, z=0.0):
    """Front-facing right triangle, legs along +x and +y from (x0, y0)."""
    return [at(x0, y0, z), at(x0, y0 + L, z), at(x0 + L, y0, z)]


def right_tri_mask(x0, y0, L, n=16):
    """Integer x0, y0, L: left and top edges own the centres on them (none lie there), the hypotenuse runs down and does not."""
    j, i = np.mgrid[0:n, 0:n]
    return (i >= x0) & (j >= y0) & (i + j + 1 < x0 + y0 + L)


def compare(got, ref, verts, tag=""):
    """The issue's rules for one mesh: got = (image, face_id, depth) of the kernel, ref = render_ref.Result."""
    img, fid, depth = got
    cov = ref.face_id >= 0
    assert np.array_equal(fid >= 0, cov), f"{tag}: coverage differs at {int(((fid >= 0) != cov).sum())} pixels"
    same = cov & (fid == ref.face_id)
    odd = np.argwhere(cov & ~same)
    zmax = float(np.abs(np.asarray(verts, np.float64)[:, 2]).max())
    for j, i in odd:
        inside, d = ref.covers(int(j), int(i), int(fid[j, i]))
        assert inside and abs(d - ref.depth[j, i]) <= 1e-6 * zmax, (tag, int(j), int(i), int(fid[j, i]), int(ref.face_id[j, i]), d, ref.depth[j, i])
    print(f"{tag}: covered {int(cov.sum())}, other face within 1e-6 max|Z| at {len(odd)}")
    assert len(odd) <= 1e-3 * cov.sum(), (tag, len(odd), int(cov.sum()))
    assert np.all(np.isinf(depth[~cov])) and np.all(fid[~cov] == -1)
    rd = np.abs(depth[same] - ref.depth[same]) / np.abs(ref.depth[same])
    assert rd.max(initial=0) <= 1e-5, (tag, float(rd.max()))
    di = np.abs(img.astype(np.int32) - ref.image.astype(np.int32))
    assert di[same].max(initial=0) <= 1, (tag, int(di[same].max()))
    assert np.array_equal(img[~cov], ref.image[~cov]), tag


# ---------------------------------------------------------------------------- known answers, 16 x 16
def test_known_single_triangle(dev):
    faces = np.array([[0, 1, 2]])
    img, fid, depth, _ = rasterize(dev, right_tri(2, 2, 10, z=0.25), faces, UNIT16, 16, 16)
    want = right_tri_mask(2, 2, 10)
    assert np.array_equal(fid >= 0, want) and want.sum() == 45
    assert np.all(fid[want] == 0) and np.allclose(depth[want], 0.25, rtol=1e-6) and np.all(np.isinf(depth[~want]))
    assert np.all(img[~want] == 0)                                   # NULL background: black where nothing is drawn
    assert np.all(img[want] > 0)                                     # ambient 0.3 at the least
    bg = np.random.default_rng(0).integers(0, 256, (16, 16, 3), dtype=np.uint8)
    img2, fid2, _, _ = rasterize(dev, right_tri(2, 2, 10, z=0.25), faces, UNIT16, 16, 16, bg=bg)
    assert np.array_equal(img2[~want], bg[~want]) and np.array_equal(img2[want], img[want]) and np.array_equal(fid2, fid)


def test_known_square_shared_diagonal(dev):
    """Two triangles sharing the diagonal (2,2)-(12,12), which passes through ten pixel centres: every pixel of the square
    is drawn exactly once, and the diagonal goes to the face for which it is a LEFT edge (face 1, the upper-right one)."""
    verts = [at(2, 2), at(2, 12), at(12, 12), at(12, 2)]
    faces = np.array([[0, 1, 2], [0, 2, 3]])
    _, fid, _, _ = rasterize(dev, verts, faces, UNIT16, 16, 16)
    j, i = np.mgrid[0:16, 0:16]
    sq = (i >= 2) & (i < 12) & (j >= 2) & (j < 12)
    want = np.where(sq, np.where(j > i, 0, 1), -1)
    assert np.array_equal(fid, want)
    ref = RR.render(verts, faces, UNIT16, 16, 16, keep_covering=True)
    assert np.array_equal(ref.face_id, want) and all(len(c) == 1 for c in ref.covering.values()) and len(ref.covering) == 100


def test_known_centre_on_vertex_and_edge(dev):
    """Corners on pixel centres: the top and the left edge own the centres on them - the corner pixel (2, 2) included - and the
    hypotenuse, which runs down, does not (nor the two corners on it)."""
    verts = [at(2.5, 2.5), at(2.5, 10.5), at(10.5, 2.5)]
    _, fid, _, _ = rasterize(dev, verts, np.array([[0, 1, 2]]), UNIT16, 16, 16)
    j, i = np.mgrid[0:16, 0:16]
    want = (i >= 2) & (j >= 2) & (i + j <= 11)
    assert np.array_equal(fid >= 0, want) and fid[2, 2] == 0 and fid[2, 10] == -1 and fid[10, 2] == -1 and fid[2, 9] == 0 and fid[9, 2] == 0


def test_known_culled_faces(dev):
    tri = right_tri(2, 2, 10)
    bg = np.full((16, 16, 3), 77, np.uint8)
    for verts, faces in ((tri, [[0, 2, 1]]),                                    # reversed winding
                         (tri, [[0, 1, 1]]),                                    # two equal corners
                         ([at(2, 2), at(5, 5), at(11, 11)], [[0, 1, 2]]),       # collinear
                         (right_tri(20, 20, 5), [[0, 1, 2]]), (right_tri(-30, 3, 12), [[0, 1, 2]])):   # wholly off the image
        img, fid, depth, _ = rasterize(dev, verts, np.array(faces), UNIT16, 16, 16, bg=bg)
        assert np.all(fid == -1) and np.all(np.isinf(depth)) and np.array_equal(img, bg)


@pytest.mark.parametrize("x0,y0", [(-5, 3), (3, -5), (10, 2), (2, 10), (-4, -4)], ids=["left", "top", "right", "bottom", "all"])
def test_known_border_crossing(dev, x0, y0):
    L = 40 if (x0, y0) == (-4, -4) else 12
    _, fid, _, _ = rasterize(dev, right_tri(x0, y0, L), np.array([[0, 1, 2]]), UNIT16, 16, 16)
    want = right_tri_mask(x0, y0, L)
    assert np.array_equal(fid >= 0, want) and 0 < want.sum() <= 256


def test_known_overlap_and_coincident(dev):
    # face 1 is nearer (smaller Z) on the overlap although it comes second; faces 2 and 3 coincide: the lower index wins
    verts = right_tri(2, 2, 10, z=0.5) + right_tri(4, 4, 10, z=0.25)
    _, fid, depth, _ = rasterize(dev, verts, np.array([[0, 1, 2], [3, 4, 5]]), UNIT16, 16, 16)
    a, b = right_tri_mask(2, 2, 10), right_tri_mask(4, 4, 10)
    assert (a & b).sum() > 0 and np.array_equal(fid, np.where(b, 1, np.where(a, 0, -1)))
    assert np.allclose(depth[b], 0.25) and np.allclose(depth[a & ~b], 0.5)
    _, fid, _, _ = rasterize(dev, right_tri(2, 2, 10), np.array([[0, 2, 1], [0, 1, 2], [0, 1, 2]]), UNIT16, 16, 16)
    assert np.array_equal(fid, np.where(a, 1, -1))


def test_known_unordered_depth_and_far_corners(dev):
    """A face with a corner whose Z is NaN or infinite is dropped, whatever its place in the list (every depth compared is
    ordered: equal bytes from two launches hold for any input); corners 2^31 snapped units apart are within the int64 range."""
    a = right_tri_mask(2, 2, 10)
    for bad in (np.nan, np.inf, -np.inf):
        tri_bad = right_tri(2, 2, 10, z=0.1)
        tri_bad[1][2] = bad
        for order in ([[0, 1, 2], [3, 4, 5]], [[3, 4, 5], [0, 1, 2]]):
            _, fid, depth, _ = rasterize(dev, tri_bad + right_tri(2, 2, 10, z=0.5), np.array(order), UNIT16, 16, 16)
            good = order.index([3, 4, 5])
            assert np.array_equal(fid, np.where(a, good, -1)) and np.allclose(depth[a], 0.5)
    # |snapped coordinate| = 2^30 exactly at both ends (16 x 16: u = 8 (1 + X) * 256): a sliver across the whole image
    far = float(2 ** 30) / 2048.0
    verts = [[-far - 1.0, -far - 1.0, 0.3], [far - 1.0, far - 1.0 - 2.0 ** -4, 0.3], [far - 1.0, far - 1.0, 0.3]]
    drawn = 0
    for faces in ([[0, 1, 2]], [[0, 2, 1]]):
        got = rasterize(dev, verts, np.array(faces), UNIT16, 16, 16)
        ref = RR.render(verts, np.array(faces), UNIT16, 16, 16)
        assert ref.ok.all() and np.abs(ref.xy).max() == 2 ** 30 and np.array_equal(got[1], ref.face_id)
        drawn += int((got[1] >= 0).sum())
    assert drawn == 16                       # the centres on the image's diagonal, under the winding that faces the camera


# ---------------------------------------------------------------------------- against render_ref
_REF = {}


def ref_of(key, verts, faces, cam, H, W, bg, color):
    """One reference per case, shared by the emulator and the GPU run of a session; never modified."""
    if key not in _REF:
        _REF[key] = [RR.render(verts[k], faces, cam[k], H, W, None if bg is None else bg[k], color) for k in range(len(verts))]
    return _REF[key]


@pytest.mark.parametrize("level,H,W,ncam", [(1, 64, 64, 1), (2, 64, 64, 1), (1, 45, 70, 1), (2, 45, 70, 1), (1, 64, 64, 3), (2, 48, 40, 3)])
def test_icosphere_matches_reference(dev, level, H, W, ncam):
    verts, faces, cams, bg = sphere_case(level, H, W, ncam)
    color = (205 / 255.0, 129 / 255.0, 98 / 255.0)
    assert len(faces) == 20 * 4 ** level
    img, fid, depth, vn = rasterize(dev, verts, faces, cams, H, W, bg=bg, color=color)
    img2, fid2, depth2, _ = rasterize(dev, verts, faces, cams, H, W, bg=bg, color=color)
    assert img.tobytes() == img2.tobytes() and fid.tobytes() == fid2.tobytes() and depth.tobytes() == depth2.tobytes()
    refs = ref_of(("sphere", level, H, W, ncam), verts, faces, cams, H, W, bg, color)
    for k in range(ncam):
        assert (refs[k].face_id >= 0).sum() > 0.1 * H * W
        compare((img[k], fid[k], depth[k]), refs[k], verts[k], tag=f"sphere{level} {W}x{H} cam{k}")
        assert np.abs(vn[k] - refs[k].vertex_normals).max() < 1e-5
        centred = verts[k] - np.array([0, 0, ZOFF], np.float32)
        assert np.abs(vn[k] - centred / np.linalg.norm(centred, axis=1, keepdims=True)).max() < 0.05       # a sphere's normals


def test_replica_indexing(dev):
    """Mesh k of a five-mesh launch = the same mesh drawn alone, byte for byte."""
    v, f = icosphere(1)
    rng = np.random.default_rng(9)
    verts = np.stack([v * s for s in (1.0, 0.7, 0.5, 0.9, 0.3)]).astype(np.float32)
    cams = np.concatenate([rng.uniform(0.5, 1.2, (5, 2)), rng.uniform(-0.4, 0.4, (5, 2))], 1).astype(np.float32)
    bg = rng.integers(0, 256, (5, 37, 50, 3), dtype=np.uint8)
    img, fid, depth, vn = rasterize(dev, verts, f, cams, 37, 50, bg=bg)
    assert len({fid[k].tobytes() for k in range(5)}) == 5
    for k in range(5):
        i1, f1, d1, n1 = rasterize(dev, verts[k:k + 1], f, cams[k:k + 1], 37, 50, bg=bg[k:k + 1])
        assert i1[0].tobytes() == img[k].tobytes() and f1[0].tobytes() == fid[k].tobytes() and d1[0].tobytes() == depth[k].tobytes()
        assert n1[0].tobytes() == vn[k].tobytes()


def check_smpl(dev, smpl_tabs, nfaces):
    verts, faces, cams = smpl_case(dev, smpl_tabs, nfaces)
    bg = np.random.default_rng(3).integers(0, 256, (2, 224, 224, 3), dtype=np.uint8)
    img, fid, depth, vn = rasterize(dev, verts, faces, cams, 224, 224, bg=bg)
    img2, fid2, depth2, _ = rasterize(dev, verts, faces, cams, 224, 224, bg=bg)
    assert img.tobytes() == img2.tobytes() and fid.tobytes() == fid2.tobytes() and depth.tobytes() == depth2.tobytes()
    # the vertices come from the skinning kernel of the device under test (fp32 sums in its own order): the reference is made from them
    refs = [RR.render(verts[k], faces, cams[k], 224, 224, bg[k]) for k in range(2)]
    for k in range(2):
        assert (refs[k].face_id >= 0).sum() > 5000
        compare((img[k], fid[k], depth[k]), refs[k], verts[k], tag=f"smpl[{nfaces}] pose{k}")
        assert np.abs(vn[k] - refs[k].vertex_normals).max() < 1e-5


def test_synthetic_smpl_matches_reference(emu_lib, smpl_tabs):
    """The synthetic SMPL's faces are random vertex triples: hundreds of front faces over every covered pixel, thousands over a
    tile - the chunked face list is what this stresses.  The first 2000 faces on the emulator (the full mesh takes it a minute)."""
    check_smpl("cpu", smpl_tabs, 2000)


@pytest.mark.gpu
def test_synthetic_smpl_matches_reference_gpu(smpl_tabs):
    check_smpl("cuda:0", smpl_tabs, 13776)


# ---------------------------------------------------------------------------- error codes
def test_error_codes_write_nothing(dev):
    from dynaboa_amd import _lib
    lib = _lib.load()
    v, f = icosphere(0)
    from dynaboa_amd.render import vertex_face_csr
    ptr, idx = vertex_face_csr(f, len(v))
    T = lambda a: torch.as_tensor(a).to(dev)
    verts, faces, ptr, idx = T(np.tile(v[None], (65, 1, 1))), T(f.astype(np.int32)), T(ptr), T(idx)
    cam = T(np.tile(np.array([[1, 1, 0, 0]], np.float32), (65, 1)))
    out = torch.full((65 * 16 * 16 * 3,), 91, dtype=torch.uint8, device=dev)
    fid = torch.full((65 * 16 * 16,), 91, dtype=torch.int32, device=dev)
    dep = torch.full((65 * 16 * 16,), 91.0, dtype=torch.float32, device=dev)
    ws = torch.full((int(lib.dyb_render_workspace_bytes(65, len(v), len(f))),), 91, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream if dev != "cpu" else None

    def call(N, H, W, wsb, out_ptr=None):
        return lib.dyb_render_meshes(verts.data_ptr(), faces.data_ptr(), ptr.data_ptr(), idx.data_ptr(), cam.data_ptr(), None, 1.0, 1.0, 1.0,
                                     out.data_ptr() if out_ptr is None else out_ptr, fid.data_ptr(), dep.data_ptr(), N, len(v), len(f), H, W,
                                     ws.data_ptr(), wsb, st)
    assert call(65, 16, 16, ws.numel()) == -3                                  # more than 64 meshes
    assert call(1, 5000, 16, ws.numel()) == -3 and call(1, 16, 4097, ws.numel()) == -3
    assert call(2, 16, 16, int(lib.dyb_render_workspace_bytes(2, len(v), len(f))) - 1) == -4
    assert call(0, 16, 16, ws.numel()) == -1 and call(1, 0, 16, ws.numel()) == -1 and call(1, 16, 16, ws.numel(), out_ptr=0) == -1
    if dev != "cpu":
        torch.cuda.synchronize()
    assert bool((out == 91).all()) and bool((fid == 91).all()) and bool((dep == 91).all()) and bool((ws == 91).all())
    assert call(2, 16, 16, ws.numel()) == 0
    if dev != "cpu":
        torch.cuda.synchronize()
    assert bool((out[:2 * 768] != 91).any()) and bool((out[2 * 768:] == 91).all())


def test_renderer_surface(dev):
    from dynaboa_amd.render import Renderer
    v, f = icosphere(1)
    with pytest.raises(NotImplementedError):
        Renderer(wireframe=True, faces=f)
    with pytest.raises(ValueError):
        Renderer()
    r = Renderer(resolution=(40, 24), faces=f, device=dev)
    cam = np.array([0.5, 0.8, 0.1, 0.0], np.float32)
    bg = np.full((24, 40, 3), 9, np.uint8)
    a = r.render(bg, v, cam, color=[0.2, 0.9, 0.4])                                 # numpy in, one mesh -> numpy (H, W, 3)
    assert isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.shape == (24, 40, 3)
    b = r.render(torch.as_tensor(bg).to(dev)[None], torch.as_tensor(v).to(dev)[None], torch.as_tensor(cam).to(dev)[None], color=[0.2, 0.9, 0.4])
    assert torch.is_tensor(b) and b.dtype == torch.uint8 and tuple(b.shape) == (1, 24, 40, 3) and b.device.type == torch.device(dev).type
    assert np.array_equal(b[0].cpu().numpy(), a) and (a != 9).any() and (a == 9).any()
    three, four = r.rasterize(v, cam, bg), r.rasterize(v, cam, bg, return_normals=True)            # the normals come on request only
    assert len(three) == 3 and len(four) == 4 and four[3].shape == v.shape and not hasattr(r, "last_vertex_normals")
    with pytest.raises(ValueError):
        r.render(bg[:, :30], v, cam)
    with pytest.raises(ValueError):
        r.render(bg, v[:5], cam)


# ---------------------------------------------------------------------------- GPU only
def test_convert_crop_cam_hand_values():
    from dynaboa_amd.render import convert_crop_cam_to_orig_img
    # s = 0.8, box 400 px high centred at (1200, 300) in a 1920 x 1080 frame:
    #   sx = 0.8 * 400 / 1920 = 1/6, sy = 0.8 * 400 / 1080 = 8/27, tx = (1200 - 960) / 960 / sx + 0.1 = 1.6, ty = (300 - 540) / 540 / sy - 0.2 = -1.7
    cam, bbox = np.array([[0.8, 0.1, -0.2]]), np.array([[1200.0, 300.0, 400.0]])
    want = np.array([[1.0 / 6.0, 8.0 / 27.0, 1.6, -1.7]])
    assert np.allclose(convert_crop_cam_to_orig_img(cam, bbox, 1920, 1080), want, rtol=1e-12)
    got = convert_crop_cam_to_orig_img(torch.tensor(cam), torch.tensor(bbox), 1920, 1080)
    assert torch.is_tensor(got) and tuple(got.shape) == (1, 4) and np.allclose(got.numpy(), want, rtol=1e-12)
    # the box is the whole (square) frame: the camera is unchanged
    assert np.allclose(convert_crop_cam_to_orig_img(np.array([[0.9, 0.3, 0.2]]), np.array([[112.0, 112.0, 224.0]]), 224, 224), [[0.9, 0.9, 0.3, 0.2]])


@pytest.mark.gpu
def test_full_hd_frame_gpu():
    """1920 x 1080, a 320-face sphere under the camera convert_crop_cam_to_orig_img gives for a 500 px box: 16-byte rows, 8160 tiles."""
    from dynaboa_amd.render import convert_crop_cam_to_orig_img
    v, f = icosphere(2)
    v[:, 2] += ZOFF
    cam = convert_crop_cam_to_orig_img(np.array([[0.9, 0.05, -0.1]]), np.array([[1300.0, 420.0, 500.0]]), 1920, 1080).astype(np.float32)
    rng = np.random.default_rng(2)
    bg = rng.integers(0, 256, (1, 1080, 1920, 3), dtype=np.uint8)
    img, fid, depth, _ = rasterize("cuda:0", v[None], f, cam, 1080, 1920, bg=bg)
    ref = RR.render(v, f, cam[0], 1080, 1920, bg[0])
    assert (ref.face_id >= 0).sum() > 100000
    compare((img[0], fid[0], depth[0]), ref, v, tag="1920x1080")
