"""The ragged overlay launch (dyb_render_meshes_var, Renderer.render_many): up to 64 meshes, each over a frame of its own size, in one
call - on the kernel emulator here, on cuda:0 under `-m gpu`.

The contract is equality of bytes: mesh i of a ragged call equals dyb_render_meshes called alone with that mesh, H_i, W_i (which
tests/test_render.py pins against its numpy reference).  Nothing here has a tolerance.

One ragged call has ONE face table.  "Icospheres of level 1, 2, 1" are therefore all given in the level-2 table (162 vertices, 320
faces): a level-1 sphere keeps its 42 vertices and puts the 120 level-2 vertices at the plain midpoints of its edges, so each of
its 80 flat faces is drawn as four coplanar ones - the level-1 surface exactly."""
import ctypes

import numpy as np
import pytest
import torch

from render_cases import (COLOR, backgrounds, corner_tile, dev, emu_lib, icosphere, ragged, shifted, smpl_case, sphere_set,      # noqa: F401 (fixtures)
                          three_spheres_three_sizes)

# ---------------------------------------------------------------------------- helpers
def uniform(dev, faces, verts, cam, bg):
    """dyb_render_meshes alone with this mesh at the frame's own size."""
    from dynaboa_amd.render import Renderer
    H, W = bg.shape[:2]
    r = Renderer(resolution=(W, H), faces=faces, device=dev)
    return r.render(torch.as_tensor(bg).to(dev), torch.as_tensor(verts).to(dev), torch.as_tensor(cam).to(dev), color=COLOR).cpu().numpy()


# ---------------------------------------------------------------------------- the contract
def test_three_spheres_three_frame_sizes_equal_uniform_calls(dev):
    """Levels 1, 2, 1 over 64 x 64 (16-byte rows: the `wide` path), 45 x 70 and 48 x 40 (H x W; neither width a multiple of 16),
    random frames, three cameras, one call."""
    faces, meshes, cams, bgs = three_spheres_three_sizes()
    got = ragged(dev, faces, meshes, cams, bgs)
    nobox = ragged(dev, faces, meshes, cams, bgs, box=False)          # flags bit 0: no per-mesh box, the same bytes
    assert [g.tobytes() for g in got] == [g.tobytes() for g in nobox]
    for k in range(3):
        want = uniform(dev, faces, meshes[k], cams[k], bgs[k])
        assert got[k].shape == bgs[k].shape and got[k].tobytes() == want.tobytes(), k
        drawn = (want != bgs[k]).any(-1).sum()
        assert 100 < drawn < 0.9 * bgs[k].shape[0] * bgs[k].shape[1], (k, int(drawn))


def test_mesh_off_its_frame_gives_back_the_frame(dev):
    flat, round2, faces = sphere_set()
    bgs = backgrounds([(40, 56), (32, 32)], seed=1)
    meshes = [shifted(round2), shifted(flat)]
    cams = [[0.5, 0.5, 7.0, 0.0], [0.6, 0.6, 0.0, 0.0]]                # mesh 0: three frame widths to the right
    got = ragged(dev, faces, meshes, cams, bgs)
    assert got[0].tobytes() == bgs[0].tobytes()
    assert got[1].tobytes() == uniform(dev, faces, meshes[1], cams[1], bgs[1]).tobytes() and (got[1] != bgs[1]).any()


def test_mesh_on_one_corner_tile_only(dev):
    """A small sphere inside the top-left 16 x 16 tile of a 48 x 40 frame: the mesh's pixel box ends inside tile (0, 0), every other
    tile of the frame lies outside it and takes the skip path - both sides of the box edge in one picture."""
    faces, mesh, cam, bg = corner_tile()
    got = ragged(dev, faces, [mesh], [cam], [bg])[0]
    assert got.tobytes() == uniform(dev, faces, mesh, cam, bg).tobytes()
    drawn = (got != bg).any(-1)
    assert drawn[:16, :16].sum() > 40 and not drawn[16:].any() and not drawn[:, 16:].any()


def test_every_face_culled_gives_back_the_frame(dev):
    _, round2, faces = sphere_set()
    # the faces that look at the camera (model-space normal with negative Z, clear of edge-on), wound the other way: all back faces
    n = np.cross(round2[faces[:, 1]] - round2[faces[:, 0]], round2[faces[:, 2]] - round2[faces[:, 0]])
    front = faces[n[:, 2] < -0.05 * np.linalg.norm(n, axis=1)][:, ::-1].copy()
    assert len(front) > 100
    bgs = backgrounds([(33, 47), (16, 16)], seed=3)
    cams = [[0.6, 0.6, 0.0, 0.0], [0.6, 0.6, 0.0, 0.0]]
    got = ragged(dev, front, [shifted(round2), shifted(round2)], cams, bgs)
    for k in range(2):
        assert got[k].tobytes() == bgs[k].tobytes()
        assert uniform(dev, front, shifted(round2), cams[k], bgs[k]).tobytes() == bgs[k].tobytes()


def test_single_mesh(dev):
    flat, _, faces = sphere_set()
    bg = backgrounds([(37, 53)], seed=4)[0]
    cam = [0.7, 0.9, 0.1, 0.05]
    got = ragged(dev, faces, [shifted(flat)], [cam], [bg], spread=False)
    assert len(got) == 1 and got[0].tobytes() == uniform(dev, faces, shifted(flat), cam, bg).tobytes() and (got[0] != bg).any()


def test_sixty_four_meshes_and_two_calls_agree(dev):
    """The limit: 64 frames of 16 x 16, every mesh with its own scale and camera; a second call gives the same bytes."""
    v0, f0 = icosphere(0)
    rng = np.random.default_rng(5)
    meshes = [shifted(v0 * (0.5 + 0.5 * rng.random())) for _ in range(64)]
    cams = [[0.5 + 0.4 * rng.random(), 0.5 + 0.4 * rng.random(), 0.6 * rng.random() - 0.3, 0.6 * rng.random() - 0.3] for _ in range(64)]
    bgs = backgrounds([(16, 16)] * 64, seed=6)
    got = ragged(dev, f0, meshes, cams, bgs)
    again = ragged(dev, f0, meshes, cams, bgs)
    assert [g.tobytes() for g in got] == [g.tobytes() for g in again]
    from dynaboa_amd.render import Renderer
    r = Renderer(resolution=(16, 16), faces=f0, device=dev)
    T = lambda a, dt: torch.as_tensor(np.asarray(a, dt)).to(dev)
    want = r.render(T(np.stack(bgs), np.uint8), T(np.stack(meshes), np.float32), T(cams, np.float32), color=COLOR).cpu().numpy()
    for k in range(64):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert sum(int((g != b).any()) for g, b in zip(got, bgs)) == 64


def test_synthetic_smpl_two_frame_sizes(dev, smpl_tabs):
    """The synthetic SMPL (random vertex triples: thousands of faces over a tile) at 224 x 224 and 72 x 144 in one call.  The first
    2000 faces on the emulator, as tests/test_render.py does (the full mesh takes it minutes); all 13 776 on the GPU."""
    verts, faces, cams = smpl_case(dev, smpl_tabs, 2000 if dev == "cpu" else 13776)
    bgs = backgrounds([(224, 224), (72, 144)], seed=7)
    got = ragged(dev, faces, [verts[0], verts[1]], cams, bgs)
    for k in range(2):
        want = uniform(dev, faces, verts[k], cams[k], bgs[k])
        assert got[k].tobytes() == want.tobytes(), k
        assert (want != bgs[k]).any(-1).sum() > 1000


# ---------------------------------------------------------------------------- error codes
def test_error_codes_write_nothing(dev):
    from dynaboa_amd import _lib
    from dynaboa_amd.render import RenderDesc, vertex_face_csr
    lib = _lib.load()
    v, f = icosphere(0)
    ptr, idx = vertex_face_csr(f, len(v))
    T = lambda a: torch.as_tensor(a).to(dev)
    verts, faces, ptr, idx = T(shifted(v)), T(f.astype(np.int32)), T(ptr), T(idx)
    cam = T(np.tile(np.array([[0.8, 0.8, 0, 0]], np.float32), (65, 1)))
    out = torch.full((65, 16, 16, 3), 91, dtype=torch.uint8, device=dev)
    nbytes = int(lib.dyb_render_var_workspace_bytes(65, len(v), len(f)))
    assert nbytes > int(lib.dyb_render_workspace_bytes(65, len(v), len(f))) > 0
    assert lib.dyb_render_var_workspace_bytes(0, len(v), len(f)) == 0
    ws = torch.full((nbytes,), 91, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream if dev != "cpu" else None

    def call(N, wsb=nbytes, H=16, W=16, null=None, table=True):
        desc = (RenderDesc * max(N, 1))()
        for i in range(N):
            desc[i] = RenderDesc(verts.data_ptr(), None, out[i % 65].data_ptr(), H, W)
        if null is not None:
            setattr(desc[1], null, None)
        return lib.dyb_render_meshes_var(ctypes.cast(desc, ctypes.c_void_p) if table else None, faces.data_ptr(), ptr.data_ptr(),
                                         idx.data_ptr(), cam.data_ptr(), 1.0, 1.0, 1.0, N, len(v), len(f), 0, ws.data_ptr(), wsb, st)
    assert call(65) == -3                                             # DYB_ERR_UNSUPPORTED: more than 64 meshes
    assert call(2, H=4097) == -3 and call(2, W=4097) == -3
    assert call(2, null="verts") == -1 and call(2, null="out") == -1  # DYB_ERR_ARG: a NULL entry
    assert call(2, table=False) == -1 and call(0) == -1 and call(2, H=0) == -1 and call(2, W=-4) == -1
    assert call(2, wsb=int(lib.dyb_render_var_workspace_bytes(2, len(v), len(f))) - 1) == -4      # DYB_ERR_WORKSPACE
    if dev != "cpu":
        torch.cuda.synchronize()
    assert bool((out == 91).all()) and bool((ws == 91).all())
    assert call(2) == 0
    if dev != "cpu":
        torch.cuda.synchronize()
    assert bool((out[:2] != 91).any()) and bool((out[2:] == 91).all())
