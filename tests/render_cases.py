"""What the overlay test files share (test_render.py, test_render_var.py, test_render_scene.py, test_scene_compose.py,
test_render_digests.py): the emulator / GPU fixtures, the test meshes, and the cases whose output bytes are pinned by
tests/golden/g11_render_digests.json (tools/make_golden_render.py records them through this module's `digest_cases`)."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

_EMU = {}
COLOR = (205 / 255.0, 129 / 255.0, 98 / 255.0)
COLORS = [COLOR, (0.2, 0.9, 0.4), (0.35, 0.45, 1.0)]
ZOFF = 2.0          # the test meshes sit in front of Z = 0, so that "1e-5 relative" on the depth means what it says at every pixel


@pytest.fixture
def emu_lib():
    """The emulator build bound for the duration of ONE test (the GPU cases of a file must see the real library)."""
    from emu.build_emu import build
    from dynaboa_amd import _abi, _lib
    if "lib" not in _EMU:
        _EMU["lib"] = _abi.bind(ctypes.CDLL(build()))
    saved = _lib._lib
    _lib.use_library(_EMU["lib"])
    yield _EMU["lib"]
    _lib._lib = saved


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def dev(request):
    if request.param == "emu":
        request.getfixturevalue("emu_lib")
        return "cpu"
    return "cuda:0"


def T(a, dev, dt=np.float32):
    return torch.as_tensor(np.asarray(a, dt)).to(dev)


# ---------------------------------------------------------------------------- meshes
def icosphere(level):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    v, f = np.array(v), np.array(f, np.int64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    inward = (n * v[f].mean(1)).sum(1) < 0
    f[inward] = f[inward][:, ::-1]               # outward normals: the side facing the camera (towards -Z) is the front
    return v.astype(np.float32), f


def sphere_case(level, H, W, ncam):
    """The uniform entry's sphere batches: ncam turned and scaled spheres, their cameras, one random frame each."""
    v, f = icosphere(level)
    rng = np.random.default_rng(100 * level + H + ncam)
    R = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    cams = np.array([[0.8, 0.8, 0.05, -0.1], [0.5, 0.9, 0.7, 0.3], [1.6, 1.3, -0.4, 0.6]], np.float32)[:ncam]
    verts = np.stack([(v @ (R if k % 2 == 0 else R.T)).astype(np.float32) * (1.0 - 0.2 * k) for k in range(ncam)])
    verts[:, :, 2] += ZOFF
    bg = rng.integers(0, 256, (ncam, H, W, 3), dtype=np.uint8)
    return verts, f, cams, bg


def smpl_case(dev, smpl_tabs, nfaces):
    from dynaboa_amd.smpl import SMPL
    g = torch.Generator().manual_seed(5)
    pose, betas = torch.randn(2, 72, generator=g) * 0.3, torch.randn(2, 10, generator=g) * 0.5
    smpl = SMPL(tables=smpl_tabs).to(dev)
    with torch.no_grad():
        verts = smpl(betas=betas.to(dev), body_pose=pose[:, 3:].to(dev), global_orient=pose[:, :3].to(dev)).vertices.cpu().numpy()
    faces = np.asarray(smpl_tabs["faces"])[:nfaces]
    cams = []
    for k in range(2):
        lo, hi = verts[k, :, :2].min(0), verts[k, :, :2].max(0)
        s = 1.7 / float((hi - lo).max())
        cams.append([s, s * 0.9, -(lo[0] + hi[0]) / 2 + 0.02 * k, -(lo[1] + hi[1]) / 2])
    verts = verts.astype(np.float32)
    verts[:, :, 2] += ZOFF + np.abs(verts[:, :, 2]).max()
    return verts, faces, np.array(cams, np.float32)


def sphere_set():
    """-> (level-1 sphere in the level-2 table, level-2 sphere, faces of level 2)."""
    v1, f1 = icosphere(1)
    v2, f2 = icosphere(2)
    assert np.array_equal(v2[:len(v1)], v1)
    flat = v2.copy()
    edges = {(min(a, b), max(a, b)) for tri in f1 for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0]))}
    placed = 0
    for a, b in sorted(edges):
        mid = (v1[a].astype(np.float64) + v1[b]) / 2
        k = int(np.argmin(np.linalg.norm(v2[len(v1):] - mid / np.linalg.norm(mid), axis=1))) + len(v1)
        flat[k] = mid.astype(np.float32)
        placed += 1
    assert placed == len(v2) - len(v1) == 120
    return flat, v2, f2


def shifted(v, z=3.0):
    v = np.array(v, np.float32)
    v[:, 2] += z
    return v


def sphere(level, radius=1.0, z=3.0):
    v, f = icosphere(level)
    return shifted(v * radius, z), f


def frame(H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def backgrounds(sizes, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def spread_rows(dev, meshes, spread=True):
    """The vertex rows as views at unequal strides inside one NaN-filled buffer (spread), as result-ring rows are."""
    V = meshes[0].shape[0]
    gaps = [5 + 7 * i for i in range(len(meshes))] if spread else [0] * len(meshes)
    buf = torch.full((sum(gaps) + len(meshes) * V * 3 + 3,), float("nan"), dtype=torch.float32, device=dev)
    rows, at = [], 0
    for m, g in zip(meshes, gaps):
        at += g
        buf[at:at + V * 3] = T(m, dev).reshape(-1)
        rows.append(buf[at:at + V * 3].view(V, 3))
        at += V * 3
    return rows


# ---------------------------------------------------------------------------- the calls
def rasterize(dev, verts, faces, cam, H, W, bg=None, color=(1.0, 1.0, 0.9)):
    """The uniform entry -> (image, face_id, depth, vertex normals) as numpy."""
    from dynaboa_amd.render import Renderer
    r = Renderer(resolution=(W, H), faces=faces, device=dev)
    out = r.rasterize(T(verts, dev), T(cam, dev), None if bg is None else torch.as_tensor(bg).to(dev), color, return_normals=True)
    return tuple(o.cpu().numpy() for o in out)


def ragged(dev, faces, meshes, cams, bgs, spread=True, box=True):
    """One ragged call; the vertex rows sit at unequal strides inside one larger buffer (spread)."""
    from dynaboa_amd.render import Renderer
    r = Renderer(resolution=(16, 16), faces=faces, device=dev)
    outs = r.render_many([torch.as_tensor(b).to(dev) for b in bgs], spread_rows(dev, meshes, spread), T(cams, dev), color=COLOR, box=box)
    return [o.cpu().numpy() for o in outs]


def draw(dev, faces, frames, scenes, resolution=(16, 16), rows=None):
    """One render_scenes call with ids.  rows: device views to use as the vertex rows (else the arrays are uploaded)."""
    from dynaboa_amd.render import Renderer
    r = Renderer(resolution=resolution, faces=faces, device=dev)
    k = 0
    sc = []
    for s in scenes:
        sc.append([])
        for v, cam, col in s:
            sc[-1].append((rows[k] if rows is not None else T(v, dev), T(cam, dev), col))
            k += 1
    pics, mids, fids = r.render_scenes([None if b is None else T(b, dev, np.uint8) for b in frames], sc, return_ids=True)
    return [p.cpu().numpy() for p in pics], [m.cpu().numpy() for m in mids], [f.cpu().numpy() for f in fids]


# ---------------------------------------------------------------------------- the cases of the three entries
def three_spheres_three_sizes():
    """Levels 1, 2, 1 over 64 x 64 (16-byte rows: the `wide` path), 45 x 70 and 48 x 40 (H x W; neither width a multiple of 16),
    random frames, three cameras -> (faces, meshes, cams, frames)."""
    flat, round2, faces = sphere_set()
    meshes = [shifted(flat), shifted(round2), shifted(flat * 0.8)]
    return faces, meshes, [[0.8, 0.8, 0.05, -0.1], [0.5, 0.75, -0.3, 0.2], [0.9, 0.7, 0.4, 0.35]], backgrounds([(64, 64), (45, 70), (48, 40)])


def corner_tile():
    """A small sphere inside the top-left 16 x 16 tile of a 48 x 40 frame -> (faces, mesh, cam, frame)."""
    _, round2, faces = sphere_set()
    # u = 20 (1 + sx (X + tx)), v = 24 (1 + sy (Y + ty)): centre at pixel (7, 8), radius 5 pixels
    return faces, shifted(round2), [0.25, 5.0 / 24.0, -0.65 / 0.25, -(2.0 / 3.0) / (5.0 / 24.0)], backgrounds([(48, 40)], seed=2)[0]


def three_scenes():
    """Sizes (33, 20), (16, 16), (48, 64) (H, W), mesh counts 1, 3 and 0, the second frame None (black)
    -> (faces, meshes, frames, scenes, sizes)."""
    v, faces = sphere(1)
    meshes = [(v, [0.7, 0.6, 0.1, -0.1], COLORS[0]),
              (v * np.float32(0.7), [0.8, 0.8, -0.4, 0.0], COLORS[1]), (v * np.float32(0.9), [0.6, 0.7, 0.3, 0.2], COLORS[2]),
              (v * np.float32(0.5), [0.9, 0.9, 0.0, -0.3], COLORS[0])]
    return faces, meshes, [frame(33, 20, seed=2), None, frame(48, 64, seed=3)], [meshes[:1], meshes[1:], []], [(33, 20), (16, 16), (48, 64)]


def front_mesh(front):
    """32 x 32 (four tiles).  The last listed sphere covers the whole picture (every tile leaves the walk after one mesh), or all of
    the two left tiles and a part of the right ones (the left tiles leave, the right ones go on to the mesh beneath)
    -> (faces, [under, top], frame)."""
    v, faces = sphere(2)
    under = (v, [0.7, 0.7, 0.1, -0.1], COLORS[1])
    # whole: radius 2.2 half pictures about the centre; left: radius 24 px about (0, 16) - the far corners of the left tiles lie at 21.9
    top = (v, [2.2, 2.2, 0.0, 0.0], COLORS[0]) if front == "whole" else (v, [1.5, 1.5, -1.0 / 1.5, 0.0], COLORS[0])
    return faces, [under, top], frame(32, 32, seed=5)


# ---------------------------------------------------------------------------- the pinned bytes
def _uniform_digest(dev, verts, faces, cams, H, W, bg, color):
    return dict(zip(("image", "face_id", "depth", "normals"), rasterize(dev, verts, faces, cams, H, W, bg=bg, color=color)))


def _d_uniform_narrow(dev, smpl_tabs):
    verts, faces, cams, bg = sphere_case(2, 48, 40, 3)
    return _uniform_digest(dev, verts, faces, cams, 48, 40, bg, COLOR)


def _d_uniform_wide_black(dev, smpl_tabs):
    verts, faces, cams, _ = sphere_case(2, 64, 64, 3)
    return _uniform_digest(dev, verts, faces, cams, 64, 64, None, COLOR)


def _d_uniform_smpl(dev, smpl_tabs):
    verts, faces, cams = smpl_case(dev, smpl_tabs, 2000)
    bg = np.random.default_rng(3).integers(0, 256, (2, 224, 224, 3), dtype=np.uint8)
    return _uniform_digest(dev, verts, faces, cams, 224, 224, bg, (1.0, 1.0, 0.9))


def _d_ragged(box):
    def case(dev, smpl_tabs):
        faces, meshes, cams, bgs = three_spheres_three_sizes()
        return {f"image{k}": o for k, o in enumerate(ragged(dev, faces, meshes, cams, bgs, box=box))}
    return case


def _d_ragged_corner(dev, smpl_tabs):
    faces, mesh, cam, bg = corner_tile()
    return {"image0": ragged(dev, faces, [mesh], [cam], [bg])[0]}


def _scene_digest(got):
    return {f"{name}{k}": a for name, arrs in zip(("image", "mesh_id", "face_id"), got) for k, a in enumerate(arrs)}


def _d_scenes_three(dev, smpl_tabs):
    faces, meshes, bgs, scenes, _ = three_scenes()
    return _scene_digest(draw(dev, faces, bgs, scenes, rows=spread_rows(dev, [m[0] for m in meshes])))


def _d_scenes_front_left(dev, smpl_tabs):
    faces, meshes, bg = front_mesh("left")
    return _scene_digest(draw(dev, faces, [bg], [meshes]))


def _d_scenes_empty(dev, smpl_tabs):
    _, faces = sphere(1)
    return _scene_digest(draw(dev, faces, [frame(37, 53, seed=1)], [[]]))


# case -> fn(dev, smpl_tabs) -> {array name: numpy array}; smpl_tabs = assets.make_synthetic_smpl(0)
DIGEST_CASES = {
    "uniform/sphere2 3 cams 48x40 frame": _d_uniform_narrow,
    "uniform/sphere2 3 cams 64x64 black": _d_uniform_wide_black,
    "uniform/smpl 2000 faces 224x224": _d_uniform_smpl,
    "ragged/three spheres box": _d_ragged(True),
    "ragged/three spheres no box": _d_ragged(False),
    "ragged/corner tile": _d_ragged_corner,
    "scenes/three scenes": _d_scenes_three,
    "scenes/front left": _d_scenes_front_left,
    "scenes/empty over a frame": _d_scenes_empty,
}


def digests(arrays):
    """{name: array} -> {name: SHA-256 of the array's bytes (C order), with its dtype and shape}."""
    return {k: f"{a.dtype}{list(a.shape)}:" + hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() for k, a in arrays.items()}
