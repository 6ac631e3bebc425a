"""Side views (a per-mesh model matrix), wireframe and .obj export of the mesh overlay (csrc/render.hip, dynaboa_amd/render.py) and the
driver flags built on them (--side_view, --wireframe, --save_obj): against known answers written out by hand, against
tests/render_ref_views.py (the numpy restatement of the matrix and of the wire rule) and against the renderer's own plain entries -
on the kernel emulator here, on cuda:0 under `-m gpu`.

The pin of everything that turns a mesh is dyb_render_transform_verts: a call with a matrix must equal, byte for byte, the plain call
on that entry's output, and that entry is held to the fp64 product within 4 * 2^-24 * sum |m_i| |v_i| per component (three roundings
of relative size 2^-24; the factor 4 covers the second-order terms).

The wireframe's drawn pixels and face ids are compared bit for bit with the restatement, its depth within the 1e-5 relative bound
test_render.py::compare uses for the solid path.  Its picture is compared in two ways: byte for byte with the kernel's own solid
picture wherever wireframe and solid show the same face (depth and shading are the solid path's), and at EVERY pixel with the
restatement's shading evaluated in fp32, one rounding per operation as the rule is written (render_ref_views.shade32, from the call's
own vertex normals, which are held to 1e-5 of the float64 ones as test_render.py holds them).  Against the float64 shading the
picture may differ by one count where 255 I colour falls next to a half: printed per case (`-s`) and held to the +-1 of
test_render.py::compare - on an MI355X 0 pixels for every sphere and triangle case, 4186 of 8118 wire pixels of the synthetic SMPL
(random-triple faces: ill-conditioned normals), all by 1."""
import os
import types

import numpy as np
import pytest
import torch

import render_ref as RR
import render_ref_views as RV
from render_cases import (COLOR, COLORS, T, dev, emu_lib, frame, front_mesh, icosphere, rasterize, shifted, smpl_case,      # noqa: F401 (fixtures)
                          sphere_case, three_spheres_three_sizes)

UNIT16 = (1.0, 1.0, 0.0, 0.0)          # on a 16 x 16 image: u = 8 (1 + X), exact for the coordinates used below
Y = [0, 1, 0]
SKEW = [0.3, -0.5, 0.8]
TURNS = [(90.0, Y), (270.0, Y), (37.0, SKEW)]


def at(u, v, z=0.0):
    """Model-space vertex that lands on image position (u, v) of a 16 x 16 image under UNIT16 (exact in fp32)."""
    return [u / 8.0 - 1.0, v / 8.0 - 1.0, z]


def right_tri(x0, y0, L, z=0.0):
    """Front-facing right triangle, legs along +x and +y from (x0, y0)."""
    return [at(x0, y0, z), at(x0, y0 + L, z), at(x0 + L, y0, z)]


def renderer(dev, faces, H, W, wireframe=False):
    from dynaboa_amd.render import Renderer
    return Renderer(resolution=(W, H), faces=faces, device=dev, wire=wireframe)


def raster(dev, verts, faces, cam, H, W, bg=None, color=(1.0, 1.0, 0.9), model=None, wireframe=False, normals=False):
    """The uniform entry -> (image, face_id, depth) as numpy; with `normals` the call's vertex normals as well."""
    out = renderer(dev, faces, H, W, wireframe).rasterize(T(verts, dev), T(cam, dev), None if bg is None else torch.as_tensor(bg).to(dev), color,
                                                          return_normals=normals, model=model)
    return tuple(o.cpu().numpy() for o in out)


def transform(dev, verts, models):
    """dyb_render_transform_verts: verts (N, V, 3), models (N, 3, 3) or None -> (N, V, 3) numpy."""
    from dynaboa_amd import _lib
    lib = _lib.load()
    v = T(verts, dev).contiguous()
    m = None if models is None else T(np.asarray(models, np.float32).reshape(-1, 9), dev).contiguous()
    out = torch.full_like(v, float("nan"))
    st = torch.cuda.current_stream().cuda_stream if dev != "cpu" else None
    assert lib.dyb_render_transform_verts(v.data_ptr(), None if m is None else m.data_ptr(), out.data_ptr(), v.shape[0], v.shape[1], st) == 0
    if dev != "cpu":
        torch.cuda.synchronize()
    return out.cpu().numpy()


def matrices():
    return np.stack([RV.side_matrix(a, ax) for a, ax in TURNS])


def same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---------------------------------------------------------------------------- 1. the transform entry
def test_transform_kernel(dev):
    from dynaboa_amd.render import side_view_matrix
    v, _ = icosphere(2)
    M = matrices()
    for k, (a, ax) in enumerate(TURNS):
        assert side_view_matrix(a, ax).dtype == np.float32 and np.array_equal(side_view_matrix(a, ax), M[k])      # fp64, rounded once
    # 270 degrees about Y in the turned space, carried into the raw one: x' = z, z' = -x
    assert np.allclose(M[1], [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], atol=1e-15)
    verts = np.stack([v, v * np.float32(0.7), v + np.float32(0.25)])
    got = transform(dev, verts, M)
    for k in range(3):
        want, bound = RV.transform_bound(M[k], verts[k])
        err = np.abs(got[k].astype(np.float64) - want)
        print(f"matrix {k}: max err {err.max():.3e}, max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert np.all(err <= bound)
    eye = np.tile(np.eye(3, dtype=np.float32), (3, 1, 1))
    assert transform(dev, verts, eye).tobytes() == verts.tobytes()
    assert transform(dev, verts, None).tobytes() == verts.tobytes()


# ---------------------------------------------------------------------------- 2. a matrix = the turned vertices
def test_rotation_equals_pre_rotation_one_mesh(dev):
    v, f = icosphere(2)
    v = shifted(v, 2.0)
    cam, bg = [0.5, 0.75, -0.3, 0.2], frame(45, 70, seed=4)
    for M in matrices():
        turned = transform(dev, v[None], M[None])[0]
        a = raster(dev, v, f, cam, 45, 70, bg, COLOR, model=M)
        b = raster(dev, turned, f, cam, 45, 70, bg, COLOR)
        assert same(a, b) and (a[1] >= 0).sum() > 100
    assert not same(raster(dev, v, f, cam, 45, 70, bg, COLOR, model=matrices()[2]), raster(dev, v, f, cam, 45, 70, bg, COLOR))


def test_rotation_equals_pre_rotation_batch(dev):
    verts, f, cams, bg = sphere_case(2, 48, 40, 3)
    M = matrices()
    a = raster(dev, verts, f, cams, 48, 40, bg, COLOR, model=M)
    b = raster(dev, transform(dev, verts, M), f, cams, 48, 40, bg, COLOR)
    # (the spheres stand two units in front of the origin: a quarter turn about Y carries them out of the picture - equal bytes all the same)
    assert same(a, b) and any((a[1][k] >= 0).sum() > 50 for k in range(3))


def test_render_without_a_turn_is_the_plain_render(dev):
    v, f = icosphere(2)
    v = shifted(v, 2.0)
    cam, bg = np.array([0.5, 0.75, -0.3, 0.2], np.float32), frame(45, 70, seed=4)
    r = renderer(dev, f, 45, 70)
    plain = r.render(bg, v, cam, color=COLOR)
    assert r.render(bg, v, cam, angle=0, color=COLOR).tobytes() == plain.tobytes()
    assert r.render(bg, v, cam, angle=90, axis=None, color=COLOR).tobytes() == plain.tobytes()
    assert r.render(bg, v, cam, angle=0, axis=Y, color=COLOR).tobytes() == plain.tobytes()
    assert r.render(bg, v, cam, angle=90, axis=Y, color=COLOR).tobytes() != plain.tobytes()


# ---------------------------------------------------------------------------- 3. known answer: a triangle seen edge-on
SIDE_ROWS = ["................",
             "................",
             "..#########.....",
             "..########......",
             "..#######.......",
             "..######........",
             "..#####.........",
             "..####..........",
             "..###...........",
             "..##............",
             "..#.............",
             "................",
             "................",
             "................",
             "................",
             "................"]


def test_known_side_view(dev):
    """A triangle in the plane X = 0: edge-on from the front.  Turned by 270 degrees about Y its raw Z becomes the image's X
    (x' = z, y' = y): with (Z, Y) of the corners at (2, 2), (2, 12), (12, 2) of the 16 x 16 image it is right_tri(2, 2, 10) of
    test_render.py, front-facing - the 45 pixels with i >= 2, j >= 2, i + j <= 11.  Turned by 90 degrees (x' = -z) it is that
    picture mirrored, so its winding is reversed: culled."""
    tri = [[0.0, p[1], p[0]] for p in right_tri(2, 2, 10)]
    faces = np.array([[0, 1, 2]])
    want = np.array([[c == "#" for c in row] for row in SIDE_ROWS])
    assert want.sum() == 45
    r = renderer(dev, faces, 16, 16)
    bg = np.full((16, 16, 3), 77, np.uint8)
    cam = np.array(UNIT16, np.float32)
    drawn = {a: (r.render(bg, np.array(tri, np.float32), cam, angle=a, axis=Y) != 77).any(2) for a in (0, 90, 270)}
    assert not drawn[0].any() and not drawn[90].any()
    assert np.array_equal(drawn[270], want)


# ---------------------------------------------------------------------------- 4. wireframe against the restatement
_CACHE = {}


def cached(key, make):
    """One reference (or one kernel output per device) per case, shared by the tests of a session; never modified."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def compare_wire(dev, key, verts, faces, cam, H, W, bg, color):
    """-> (wire, solid) kernel outputs, the wireframe checked against the restatement as the module docstring says."""
    wire = cached((dev, "wire", key), lambda: raster(dev, verts, faces, cam, H, W, bg, color, wireframe=True))
    solid = cached((dev, "solid", key), lambda: raster(dev, verts, faces, cam, H, W, bg, color, normals=True))
    vn = solid[3]
    ref = cached(("ref", key, vn.tobytes()), lambda: RV.render_wire(verts, faces, cam, H, W, bg, color, normals=vn))
    assert np.abs(vn - ref.vertex_normals).max() < 1e-5
    img, fid, depth = wire
    assert np.array_equal(fid, ref.face_id), f"{key}: face ids differ at {int((fid != ref.face_id).sum())} pixels"
    cov = fid >= 0
    assert np.all(np.isinf(depth[~cov])) and np.all(depth[~cov] > 0)
    rd = np.abs(depth[cov] - ref.depth[cov]) / np.abs(ref.depth[cov])
    same_face = cov & (fid == solid[1])
    di = np.abs(img.astype(np.int32) - ref.image.astype(np.int32))
    d32 = int((img != ref.image32).any(2).sum())
    print(f"{key}: wire pixels {int(cov.sum())} of {int((solid[1] >= 0).sum())} solid, depth rel err {rd.max(initial=0):.2e}, "
          f"same face as solid {int(same_face.sum())}, picture differs from the fp32 restatement at {d32} pixels, from the float64 one at "
          f"{int((di.max(2) > 0).sum())} pixels (max {int(di.max(initial=0))})")
    assert rd.max(initial=0) <= 1e-5
    assert np.array_equal(img[same_face], solid[0][same_face]) and np.array_equal(depth[same_face], solid[2][same_face])
    base = np.zeros((H, W, 3), np.uint8) if bg is None else bg
    assert np.array_equal(img[~cov], base[~cov])
    assert np.array_equal(img, ref.image32)
    assert di.max(initial=0) <= 1
    return wire, solid


def test_wire_known_triangle(dev):
    """Legs of 12 pixels from (2.25, 2.25): inside are the centres with i >= 2, j >= 2, i + j <= 15.  The left edge x = 2.25 is within
    one pixel (along x) of the centres of column 2 only, the top edge of row 2 only, and the hypotenuse x + y = 16.5 of the centres
    with i + j + 1 = 16 (half a pixel away along x; the next diagonal is 1.5 away)."""
    verts, faces = right_tri(2.25, 2.25, 12, z=0.5), np.array([[0, 1, 2]])
    bg = frame(16, 16, seed=7)
    (img, fid, depth), solid = compare_wire(dev, "tri12", verts, faces, UNIT16, 16, 16, bg, COLOR)
    j, i = np.mgrid[0:16, 0:16]
    inside = (i >= 2) & (j >= 2) & (i + j <= 15)
    bands = inside & ((i == 2) | (j == 2) | (i + j == 15))
    assert np.array_equal(solid[1] >= 0, inside) and np.array_equal(fid >= 0, bands) and bands.sum() == 12 + 11 + 10
    assert fid[5, 5] == -1 and np.isinf(depth[5, 5]) and np.array_equal(img[5, 5], bg[5, 5]) and solid[1][5, 5] == 0      # the frame shows through
    assert fid[2, 9] == 0 and fid[9, 2] == 0 and fid[7, 8] == 0 and fid[13, 2] == 0 and fid[2, 13] == 0


def test_wire_square_shared_diagonal(dev):
    verts = [at(2, 2, 0.5), at(2, 12, 0.5), at(12, 12, 0.5), at(12, 2, 0.5)]
    compare_wire(dev, "square", verts, np.array([[0, 1, 2], [0, 2, 3]]), UNIT16, 16, 16, frame(16, 16, seed=8), COLOR)


@pytest.mark.parametrize("x0,y0", [(-5, 3), (3, -5), (10, 2), (2, 10), (-4, -4)], ids=["left", "top", "right", "bottom", "all"])
def test_wire_border_crossing(dev, x0, y0):
    L = 40 if (x0, y0) == (-4, -4) else 12
    compare_wire(dev, ("border", x0, y0), right_tri(x0, y0, L, z=0.5), np.array([[0, 1, 2]]), UNIT16, 16, 16, frame(16, 16, seed=9), COLOR)


@pytest.mark.parametrize("level,H,W", [(1, 64, 64), (2, 64, 64), (1, 45, 70), (2, 45, 70)])
def test_wire_icosphere(dev, level, H, W):
    verts, faces, cams, bg = sphere_case(level, H, W, 1)
    wire, solid = compare_wire(dev, ("sphere", level, H, W), verts[0], faces, cams[0], H, W, bg[0], COLOR)
    assert (wire[1] >= 0).sum() > 100


@pytest.mark.gpu
def test_wire_synthetic_smpl_gpu(smpl_tabs):
    verts, faces, cams = smpl_case("cuda:0", smpl_tabs, 2000)
    bg = np.random.default_rng(3).integers(0, 256, (224, 224, 3), dtype=np.uint8)
    compare_wire("cuda:0", "smpl2000", verts[0], faces, cams[0], 224, 224, bg, (1.0, 1.0, 0.9))


def test_wire_is_asked_for_by_its_own_name(dev):
    """``wire=True`` selects the wire rule; the reference's spelling ``wireframe=True`` stays refused, as tests/test_render.py pins it
    (pyrender's line rasterisation is not what is drawn)."""
    from dynaboa_amd.render import Renderer
    _, f = icosphere(1)
    assert Renderer(faces=f, wire=True).wireframe is True and Renderer(faces=f).wireframe is False
    with pytest.raises(NotImplementedError):
        Renderer(faces=f, wireframe=True)


# ---------------------------------------------------------------------------- 5. wire pixels lie inside the solid
def test_wire_inside_solid_sphere(dev):
    verts, faces, cams, bg = sphere_case(2, 64, 64, 1)
    key = ("sphere", 2, 64, 64)
    wire = cached((dev, "wire", key), lambda: raster(dev, verts[0], faces, cams[0], 64, 64, bg[0], COLOR, wireframe=True))
    solid = cached((dev, "solid", key), lambda: raster(dev, verts[0], faces, cams[0], 64, 64, bg[0], COLOR))
    w, s = wire[1] >= 0, solid[1] >= 0
    assert w.any() and not (w & ~s).any() and (s & ~w).any()


def test_wire_inside_solid_smpl(dev, smpl_tabs):
    verts, faces, cams = smpl_case(dev, smpl_tabs, 2000)
    w = raster(dev, verts[0], faces, cams[0], 224, 224, wireframe=True)[1] >= 0
    s = raster(dev, verts[0], faces, cams[0], 224, 224)[1] >= 0
    assert w.any() and not (w & ~s).any() and (s & ~w).any()


# ---------------------------------------------------------------------------- 6. the ragged and the scene entry
@pytest.mark.parametrize("wireframe", [False, True], ids=["solid", "wire"])
def test_ragged_equals_single_renders(dev, wireframe):
    from dynaboa_amd.render import side_view_matrix
    faces, meshes, cams, bgs = three_spheres_three_sizes()
    singles = []
    for v, cam, bg, (a, ax) in zip(meshes, cams, bgs, TURNS):
        r = renderer(dev, faces, bg.shape[0], bg.shape[1], wireframe)
        singles.append(r.render(bg, v, np.array(cam, np.float32), angle=a, axis=ax, color=COLOR))
    r = renderer(dev, faces, 16, 16, wireframe)
    models = [side_view_matrix(a, ax) for a, ax in TURNS]
    for box in (True, False):
        outs = r.render_many([torch.as_tensor(b).to(dev) for b in bgs], [T(m, dev) for m in meshes], T(cams, dev), color=COLOR, box=box,
                             models=models)
        for o, s in zip(outs, singles):
            assert o.cpu().numpy().tobytes() == s.tobytes()
    assert any((s != bg).any() for s, bg in zip(singles, bgs))       # (a quarter turn about Y carries a sphere at Z = 3 out of its picture)
    plain = r.render_many([torch.as_tensor(b).to(dev) for b in bgs], [T(m, dev) for m in meshes], T(cams, dev), color=COLOR)
    assert any(p.cpu().numpy().tobytes() != s.tobytes() for p, s in zip(plain, singles))
    # a matrix for one mesh only: the others are drawn as they are
    one = r.render_many([torch.as_tensor(b).to(dev) for b in bgs], [T(m, dev) for m in meshes], T(cams, dev), color=COLOR,
                        models=[None, models[1], None])
    assert [o.cpu().numpy().tobytes() == p.cpu().numpy().tobytes() for o, p in zip(one, plain)] == [True, False, True]
    assert one[1].cpu().numpy().tobytes() == singles[1].tobytes()


def test_scene_wire_equals_chain(dev):
    """Two overlapping meshes, the upper one turned, wireframe: the upper mesh covers the two left tiles of the picture as a solid,
    but claims its wire pixels only - those tiles must go on to the mesh beneath."""
    from dynaboa_amd.render import side_view_matrix
    faces, (under, top), bg = front_mesh(False)
    Z = [0, 0, 1]                                                    # about Z the sphere turns in place: it goes on covering the left tiles
    M = side_view_matrix(37.0, Z)
    r = renderer(dev, faces, 32, 32, wireframe=True)
    chain = r.render(bg, under[0], np.array(under[1], np.float32), color=under[2])
    only_under = chain.copy()
    chain = r.render(chain, top[0], np.array(top[1], np.float32), angle=37.0, axis=Z, color=top[2])
    pics, mids, fids = r.render_scenes([T(bg, dev, np.uint8)], [[(T(under[0], dev), T(under[1], dev), under[2]),
                                                                  (T(top[0], dev), T(top[1], dev), top[2], M)]], return_ids=True)
    assert pics[0].cpu().numpy().tobytes() == chain.tobytes()
    mid = mids[0].cpu().numpy()
    assert (mid == 0).any() and (mid == 1).any() and (mid == -1).any()
    # in the two left tiles, which the upper mesh covers wholly as a solid, the mesh beneath still shows
    solid_top = renderer(dev, faces, 32, 32).rasterize(T(top[0], dev), T(top[1], dev), model=M)[1].cpu().numpy() >= 0
    assert solid_top[:, :16].all() and (mid[:, :16] == 0).any() and (chain != only_under).any()


# ---------------------------------------------------------------------------- 7. errors write nothing
def test_bad_matrix_writes_nothing(dev):
    from dynaboa_amd import _lib
    from dynaboa_amd.render import RenderDesc, RenderOpts, vertex_face_csr
    import ctypes
    lib = _lib.load()
    v, f = icosphere(0)
    ptr, idx = vertex_face_csr(f, len(v))
    N, V, F = 2, len(v), len(f)
    verts, faces, ptr, idx = T(np.tile(shifted(v)[None], (N, 1, 1)), dev), T(f, dev, np.int32), T(ptr, dev, np.int32), T(idx, dev, np.int32)
    cam = T(np.tile(np.array([[1, 1, 0, 0]], np.float32), (N, 1)), dev)
    out = torch.full((N * 16 * 16 * 3,), 91, dtype=torch.uint8, device=dev)
    fid = torch.full((N * 16 * 16,), 91, dtype=torch.int32, device=dev)
    dep = torch.full((N * 16 * 16,), 91.0, dtype=torch.float32, device=dev)
    need = int(lib.dyb_render_var_workspace_bytes(N, V, F)) + int(lib.dyb_render_model_workspace_bytes(N, V))
    assert int(lib.dyb_render_model_workspace_bytes(N, V)) >= N * V * 12
    ws = torch.full((need,), 91, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream if dev != "cpu" else None
    desc = (RenderDesc * N)(*[RenderDesc(verts[n].data_ptr(), None, out[n * 768:].data_ptr(), 16, 16) for n in range(N)])

    def calls(model, wsb=need, which=(0, 1)):
        o = RenderOpts(model.data_ptr(), 0)
        a = 0 not in which or lib.dyb_render_meshes_opt(verts.data_ptr(), faces.data_ptr(), ptr.data_ptr(), idx.data_ptr(), cam.data_ptr(), None, 1.0, 1.0, 1.0,
                                      out.data_ptr(), fid.data_ptr(), dep.data_ptr(), N, V, F, 16, 16, ws.data_ptr(), wsb, st, ctypes.addressof(o))
        b = 1 not in which or lib.dyb_render_meshes_var_opt(ctypes.cast(desc, ctypes.c_void_p), faces.data_ptr(), ptr.data_ptr(), idx.data_ptr(), cam.data_ptr(),
                                          1.0, 1.0, 1.0, N, V, F, 0, ws.data_ptr(), wsb, st, ctypes.addressof(o))
        return a, b
    good = np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (N, 1))
    for bad in (np.nan, np.inf, -np.inf):
        m = good.copy()
        m[1, 5] = bad                                                # the last mesh's matrix: every matrix is looked at
        assert calls(T(m, dev)) == (-1, -1)
    # the turned rows need their own room behind the entry's scratch
    assert calls(T(good, dev), wsb=need - 1, which=(1,))[1] == -4
    assert calls(T(good, dev), wsb=int(lib.dyb_render_workspace_bytes(N, V, F)) + int(lib.dyb_render_model_workspace_bytes(N, V)) - 1, which=(0,))[0] == -4
    if dev != "cpu":
        torch.cuda.synchronize()
    assert bool((out == 91).all()) and bool((fid == 91).all()) and bool((dep == 91).all()) and bool((ws == 91).all())
    assert calls(T(good, dev)) == (0, 0)
    if dev != "cpu":
        torch.cuda.synchronize()
    assert bool((out != 91).any()) and bool((fid != 91).any())
    # the Python surface reports it too
    with pytest.raises(RuntimeError, match="bad argument"):
        raster(dev, shifted(v), f, [1, 1, 0, 0], 16, 16, model=np.full((3, 3), np.nan, np.float32))


# ---------------------------------------------------------------------------- 8. .obj
def test_obj_round_trip(dev, tmp_path):
    v, f = icosphere(1)
    v = (shifted(v) * np.float32(1.0 / 3.0)).astype(np.float32)      # thirds: no short decimal form
    cam, bg = np.array([0.5, 0.8, 0.1, 0.0], np.float32), np.full((24, 40, 3), 9, np.uint8)
    r = renderer(dev, f, 24, 40)
    a = r.render(bg, v, cam, mesh_filename=str(tmp_path / "a.obj"))
    b = r.render(bg, T(v, dev), T(cam, dev), angle=270, axis=Y, mesh_filename=str(tmp_path / "b.obj"))
    assert a.tobytes() == r.render(bg, v, cam).tobytes() and b.cpu().numpy().tobytes() != a.tobytes()
    pv, pf = RV.parse_obj(tmp_path / "a.obj")
    assert pv.tobytes() == (v * np.array([1, -1, -1], np.float32)).tobytes()
    assert np.array_equal(pf, np.asarray(f) + 1) and pf.min() == 1
    assert open(tmp_path / "a.obj", "rb").read() == open(tmp_path / "b.obj", "rb").read()      # written before the turn
    with pytest.raises(ValueError):
        r.render(bg[None], v[None], cam[None], mesh_filename=str(tmp_path / "c.obj"))
    assert not os.path.exists(tmp_path / "c.obj")


# ---------------------------------------------------------------------------- 9. save_results: the panel
NFACES_PANEL = 600          # the synthetic bundle's mesh with its first faces only: the emulator draws every picture here several times


def panel_adaptor(dev, smpl_tabs, exppath, **flags):
    """What save_results needs of an adaptor - the synthetic bundle's neutral SMPL (its face table cut short), the options, the
    experiment folder - without the network: BaseAdaptor's own methods on a bare instance."""
    from dynaboa_amd.base_adaptor import BaseAdaptor
    ad = object.__new__(BaseAdaptor)
    ad.options = types.SimpleNamespace(**flags)
    ad.smpl_neutral = types.SimpleNamespace(faces=np.asarray(smpl_tabs["faces"])[:NFACES_PANEL])
    ad.device, ad.exppath, ad.global_step = torch.device(dev), str(exppath), 4
    return ad


def panel_inputs(dev, smpl_tabs):
    verts, _, cams = smpl_case(dev, smpl_tabs, NFACES_PANEL)
    verts[:, :, 2] -= verts[:, :, 2].mean(1, keepdims=True)          # about the origin again, as the network's meshes are: a turn keeps them in view
    g = torch.Generator().manual_seed(1)
    images = torch.randn(2, 3, 224, 224, generator=g).to(dev)
    cam = torch.tensor([[cams[0][0], cams[0][2], cams[0][3]], [cams[1][0], cams[1][2], cams[1][3]]], dtype=torch.float32, device=dev)
    return T(verts, dev), cam, images


def read_png(path):
    from PIL import Image
    return np.array(Image.open(path))


@pytest.mark.parametrize("wireframe", [0, 1], ids=["solid", "wire"])
def test_save_results_panel(dev, smpl_tabs, tmp_path, wireframe):
    from dynaboa_amd.base_adaptor import BaseAdaptor
    vts, cam, images = panel_inputs(dev, smpl_tabs)
    plain = panel_adaptor(dev, smpl_tabs, tmp_path / "plain", wireframe=wireframe)
    paths0 = plain.save_results(vts, cam, images, None, None, prefix="Pred")
    ad = panel_adaptor(dev, smpl_tabs, tmp_path / "side", side_view=270.0, wireframe=wireframe, save_obj=1)
    paths = ad.save_results(vts, cam, images, None, None, prefix="Pred")
    assert [os.path.basename(p) for p in paths] == [os.path.basename(p) for p in paths0] == ["Pred_4.png", "Pred_5.png"]
    assert not os.path.exists(tmp_path / "plain" / "mesh")
    r = renderer(dev, ad.smpl_neutral.faces, 224, 224, wireframe=bool(wireframe))
    white = np.full((224, 224, 3), 255, np.uint8)
    for k in range(2):
        left0, both = read_png(paths0[k]), read_png(paths[k])
        assert left0.shape == (224, 224, 3) and both.shape == (224, 448, 3)
        assert np.array_equal(both[:, :224], left0)
        ccam = torch.stack([cam[k, 0], cam[k, 0], cam[k, 1], cam[k, 2]])
        want = r.render(torch.as_tensor(white).to(dev), vts[k], ccam, angle=270, axis=[0, 1, 0], color=BaseAdaptor.RESULT_COLOR).cpu().numpy()
        assert np.array_equal(both[:, 224:], want) and (want != 255).any()
        crop = torch.as_tensor(left0).to(dev)            # where nothing is drawn the left half is the crop: draw over a copy of it
        front = r.render(crop, vts[k], ccam, color=BaseAdaptor.RESULT_COLOR).cpu().numpy()
        assert np.array_equal(front, left0)              # drawing the same mesh again over its own overlay changes nothing
        pv, pf = RV.parse_obj(tmp_path / "side" / "mesh" / f"Pred_{4 + k}.obj")
        assert pv.tobytes() == (vts[k].cpu().numpy() * np.array([1, -1, -1], np.float32)).tobytes()
        assert np.array_equal(pf, ad.smpl_neutral.faces + 1)
    if wireframe:
        solid = read_png(panel_adaptor(dev, smpl_tabs, tmp_path / "solid").save_results(vts, cam, images, None, None, prefix="Pred")[0])
        assert not np.array_equal(solid, read_png(paths0[0]))


def test_side_view_jobs_pack_32_people_per_launch(tmp_path):
    """65 people with side views: 130 descriptors in launches of 64, 64 and 2 - a picture's halves never in two launches."""
    from dynaboa_amd.base_adaptor import draw_overlays
    seen = []

    class Spy:
        def render_many(self, frames, rows, cams, color=None, models=None):
            seen.append((len(rows), [m is not None for m in models]))
            return [torch.zeros(2, 3, 3, dtype=torch.uint8) for _ in rows]
    jobs = []
    for k in range(65):
        jobs += [(None, None, torch.zeros(4), str(tmp_path / f"{k}.png")), (None, None, torch.zeros(4), None, np.eye(3, dtype=np.float32))]
    draw_overlays(Spy(), jobs, COLOR)
    assert [n for n, _ in seen] == [64, 64, 2] and all(flags == [False, True] * (n // 2) for n, flags in seen)


# ---------------------------------------------------------------------------- 10. the native stepper keeps the flags (GPU only)
@pytest.mark.gpu
def test_native_results_with_side_view_and_wireframe_gpu(tmp_path):
    """Two sequences, two frames: a replica group on the native stepper with --native_results 1 --save_res 1 --side_view 270
    --wireframe 1 writes the bytes the autograd path writes with the same flags."""
    import test_native_results_gpu as NR
    from dynaboa_amd import benchmark as DB, native_step as NS
    flags = dict(NR.FRAME_ONLY, deferred_metrics=0, save_res=1, side_view=270.0, wireframe=1)
    frames = NR._frames(2, 2)
    o = DB.frame_only_options()
    o.save_res, o.side_view, o.wireframe, o.save_obj = 1, 270.0, 1, 1
    assert NS.coverage(o) == ("", "rendered results")
    o.native_results = 1
    assert NS.coverage(o) == ("frame", None)
    want = []
    for r in range(2):
        ad = NR._mk(r, flags, tmp_path / f"autograd{r}")
        NR._run(ad, frames[r])
        assert ad._native is None
        want.append([open(tmp_path / f"autograd{r}" / "nr" / "image" / f"Pred_{s}.png", "rb").read() for s in range(2)])
    ads = [NR._mk(r, dict(flags, native_results=1), tmp_path / f"native{r}") for r in range(2)]
    grp = NS.ReplicaGroup(ads, 2)
    for s in range(2):
        grp.step([frames[0][s], frames[1][s]], s)
    torch.cuda.synchronize()
    for r in range(2):
        assert ads[r]._native is grp.stepper and grp.stepper.results is not None
        for s in range(2):
            path = tmp_path / f"native{r}" / "nr" / "image" / f"Pred_{s}.png"
            assert read_png(path).shape == (224, 448, 3)
            assert open(path, "rb").read() == want[r][s], (r, s)
    assert len({b for w in want for b in w}) == 4
