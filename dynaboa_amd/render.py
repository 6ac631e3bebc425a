"""Mesh overlay: the reference's ``render_demo.py`` surface - ``Renderer(resolution, orig_img, wireframe)`` with
``.render(img, verts, cam, angle, axis, mesh_filename, color)`` and ``convert_crop_cam_to_orig_img`` - on the HIP rasteriser of
csrc/render.hip.

The reference draws one frame at a time with pyrender on OpenGL through the host; here the vertices, the camera and the frame stay
on the device and a batch of meshes (one per sequence of a step, up to 64) is drawn by one call.  Geometry, visibility, the ambient
term and the three light positions are the reference's; the material model is plain smooth diffuse shading, NOT pyrender's
metallic-roughness one (unpinned: pyrender is absent from the build image).  Conventions: csrc/render.hip."""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import constants as C
from ._abi import check
from .hmr import stream_of

MAX_MESHES = 64
MAX_DIM = 4096
DEFAULT_COLOR = (1.0, 1.0, 0.9)          # render_demo.py:86


def vertex_face_csr(faces: np.ndarray, num_verts: int) -> Tuple[np.ndarray, np.ndarray]:
    """(ptr [V+1], idx [3F]) int32: the faces incident to each vertex, ascending per vertex (a face naming a vertex twice is
    listed twice under it)."""
    flat = np.asarray(faces, np.int64).reshape(-1)
    order = np.argsort(flat, kind="stable")
    ptr = np.zeros(num_verts + 1, np.int64)
    np.cumsum(np.bincount(flat, minlength=num_verts), out=ptr[1:])
    return ptr.astype(np.int32), (order // 3).astype(np.int32)


def convert_crop_cam_to_orig_img(cam, bbox, img_width, img_height):
    """Weak-perspective camera (s, tx, ty) of the square crop -> (sx, sy, tx, ty) in the original frame, for boxes (cx, cy, h)
    in frame pixels (what reference render_demo.py:136-153 computes).  cam (B, 3), bbox (B, 3); numpy or torch -> (B, 4).

    The crop shows the h x h box centred at (cx, cy).  In normalised coordinates (-1 ... 1 across an image) a crop position q
    lies at  h / (W, H) * q + (2 (cx, cy) / (W, H) - 1)  of the frame, and the crop camera puts the model point X at
    q = s (X + t).  Written again as scale * (X + shift):  scale = s h / (W, H),  shift = t + (2 (cx, cy) / (W, H) - 1) / scale."""
    if torch.is_tensor(cam):
        frame, cat = cam.new_tensor([float(img_width), float(img_height)]), torch.cat
        bbox = bbox.to(cam.device, cam.dtype)
    else:
        frame, cat = np.array([float(img_width), float(img_height)]), np.concatenate
    scale = cam[:, :1] * bbox[:, 2:3] / frame
    shift = cam[:, 1:3] + (2.0 * bbox[:, :2] / frame - 1.0) / scale
    return cat([scale, shift], 1)


class RenderDesc(ctypes.Structure):
    """dyb_render_desc (include/dynaboa_hip.h): one mesh of a ragged call."""
    _fields_ = [("verts", ctypes.c_void_p), ("background", ctypes.c_void_p), ("out", ctypes.c_void_p), ("H", ctypes.c_int),
                ("W", ctypes.c_int)]


class RenderScene(ctypes.Structure):
    """dyb_render_scene (include/dynaboa_hip.h): one scene of a scene call."""
    _fields_ = [("background", ctypes.c_void_p), ("out", ctypes.c_void_p), ("mesh_id", ctypes.c_void_p), ("face_id", ctypes.c_void_p),
                ("H", ctypes.c_int), ("W", ctypes.c_int), ("mesh_begin", ctypes.c_int), ("mesh_end", ctypes.c_int)]


class RenderOpts(ctypes.Structure):
    """dyb_render_opts (include/dynaboa_hip.h): what the _opt entries take beside the plain arguments."""
    _fields_ = [("model", ctypes.c_void_p), ("wireframe", ctypes.c_int)]


def side_view_matrix(angle, axis) -> np.ndarray:
    """The matrix the rasteriser takes (its raw model space, row major, fp32 (3, 3)) for the reference's side view: the mesh turned
    by Rx (180 degrees about X) and then by R(angle in degrees, axis) (render_demo.py:90-98).  The rasteriser folds Rx into its image
    coordinates, so it is handed Rx R Rx - formed in fp64 (Rodrigues, as trimesh.transformations.rotation_matrix) and rounded once."""
    k = np.asarray(axis, np.float64).reshape(3)
    n = float(np.linalg.norm(k))
    if not n > 0.0:
        raise ValueError("the axis of a side view must not vanish")
    k = k / n
    a = math.radians(float(angle))
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    R = math.cos(a) * np.eye(3) + math.sin(a) * K + (1.0 - math.cos(a)) * np.outer(k, k)
    Rx = np.diag([1.0, -1.0, -1.0])
    return (Rx @ R @ Rx).astype(np.float32)


def write_obj(path, verts, faces) -> None:
    """Wavefront .obj: one ``v x y z`` line per vertex with 9 significant digits (fp32 round-trips), then one 1-based ``f i j k``
    line per face."""
    v = np.asarray(verts, np.float32)
    with open(path, "w") as fh:
        fh.write("".join("v %.9g %.9g %.9g\n" % (float(x), float(y), float(z)) for x, y, z in v))
        fh.write("".join("f %d %d %d\n" % (int(a) + 1, int(b) + 1, int(c) + 1) for a, b, c in np.asarray(faces)))


def turned_vertices(verts) -> np.ndarray:
    """The mesh as the reference exports it: turned by Rx, (X, -Y, -Z), fp32 on the host."""
    v = verts.detach().cpu().numpy() if torch.is_tensor(verts) else np.asarray(verts)
    return v.astype(np.float32) * np.array([1.0, -1.0, -1.0], np.float32)


def parse_cam(cam_t):
    """The crop camera (s, tx, ty) back from the ``cam_t`` = (tx, ty, 2 f / (224 s + 1e-9)) that the ``Pred_{n}.pt`` dumps store
    (reference render_demo.py:162-166).  cam_t (B, 3), numpy or torch -> (B, 3) of the same kind."""
    stack = torch.stack if torch.is_tensor(cam_t) else np.stack
    s = (2 * C.FOCAL_LENGTH / cam_t[:, 2] - 1e-9) / C.IMG_RES
    return stack([s, cam_t[:, 0], cam_t[:, 1]], 1)


def track_color(track: int) -> Tuple[float, float, float]:
    """The colour a tracked person is drawn in: constants.TRACK_COLORS by track id modulo its length; a detection without a track
    (-1) takes entry 0, the reference's colour."""
    r, g, b = C.TRACK_COLORS[int(track) % len(C.TRACK_COLORS) if track >= 0 else 0]
    return (r / 255.0, g / 255.0, b / 255.0)


class Renderer:
    """``resolution`` is (width, height) as in the reference.  ``faces``: the (F, 3) table an ``SMPL`` carries (``smpl.faces``);
    the int32 copy and the vertex -> face adjacency are built once here.  ``device``: where numpy inputs are drawn.
    ``wire=True``: every call of this renderer draws the faces' edges only (the wire rule of csrc/render.hip; what the reference's
    RenderFlags.ALL_WIREFRAME selects).  The reference's own spelling, ``wireframe=True``, is still refused: the wire rule is this
    project's restatement, unpinned against pyrender, and a caller porting reference code must ask for it by its own name
    (tests/test_render.py pins the refusal).  ``self.wireframe`` tells which a renderer draws."""

    def __init__(self, resolution=(224, 224), orig_img=False, wireframe=False, faces=None, device=None, wire=False):
        if wireframe:
            raise NotImplementedError("pyrender's RenderFlags.ALL_WIREFRAME is not reproduced; wire=True draws this project's wire rule")
        if faces is None:
            raise ValueError("Renderer needs the mesh's face table: faces=smpl.faces")
        self.resolution = (int(resolution[0]), int(resolution[1]))
        self.orig_img = orig_img
        self.wireframe = bool(wire)
        f = faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)
        if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] == 0:
            raise ValueError("faces must be (F, 3)")
        if f.min() < 0:
            raise ValueError("negative vertex index in faces")
        self.faces = np.ascontiguousarray(f, dtype=np.int32)
        self.min_verts = int(f.max()) + 1
        self.device = torch.device(device) if device is not None else None
        self._tables: Dict[tuple, tuple] = {}
        self._ws: Dict[tuple, torch.Tensor] = {}

    def _adjacency(self, V: int, dev: torch.device):
        """(faces, vertex -> face ptr, idx) on dev for meshes of V vertices."""
        if V < self.min_verts:
            raise ValueError(f"faces index vertex {self.min_verts - 1} but the mesh has {V} vertices")
        key = (V, str(dev))
        hit = self._tables.get(key)
        if hit is None:
            ptr, idx = vertex_face_csr(self.faces, V)
            hit = self._tables[key] = tuple(torch.from_numpy(a).to(dev) for a in (self.faces, ptr, idx))
        return hit

    def _device_of(self, *xs) -> torch.device:
        for x in xs:
            if torch.is_tensor(x):
                return x.device
        if self.device is not None:
            return self.device
        return torch.device("cuda" if torch.cuda.is_available() else "cpu")

    def _workspace(self, dev: torch.device, nbytes: int) -> torch.Tensor:
        """The scratch of a call: one buffer per (device, stream), grown when a call needs more."""
        key = (str(dev), torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0)
        ws = self._ws.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = self._ws[key] = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        return ws

    def _frame(self, bg, dev: torch.device, over: str):
        """A frame (uint8 RGB (H, W, 3)) or None (black at `resolution`) -> (contiguous tensor on dev or None, H, W)."""
        if bg is None:
            W, H = self.resolution
        else:
            bg = torch.as_tensor(bg).to(dev)
            if bg.dtype != torch.uint8 or bg.dim() != 3 or bg.shape[2] != 3:
                raise ValueError(f"the frame under the {over} must be uint8 RGB (H, W, 3)")
            bg = bg.contiguous()
            H, W = int(bg.shape[0]), int(bg.shape[1])
        if not (0 < H <= MAX_DIM and 0 < W <= MAX_DIM):
            raise ValueError(f"frame size {(H, W)} outside 1 .. {MAX_DIM}")
        return bg, H, W

    @staticmethod
    def _row(v, V: int, dev: torch.device, message: str) -> torch.Tensor:
        """One mesh's vertices as a contiguous fp32 (V, 3) row on dev: the tensor itself where it already is one."""
        v = torch.as_tensor(v).detach()
        if v.dtype != torch.float32 or not v.is_contiguous() or v.device != dev:
            v = v.to(dev, torch.float32).contiguous()
        if tuple(v.shape) != (V, 3):
            raise ValueError(message)
        return v

    @staticmethod
    def _models(models, N: int, dev: torch.device) -> Optional[torch.Tensor]:
        """One 3x3 matrix (or None = identity) per mesh -> fp32 (N, 9) on dev; None when no mesh has one."""
        if models is None:
            return None
        if torch.is_tensor(models):
            m = models.detach().to(dev, torch.float32)
        else:
            if len(models) != N:
                raise ValueError(f"{len(models)} matrices for {N} meshes")
            if all(x is None for x in models):
                return None
            eye = np.eye(3, dtype=np.float32)
            rows = [eye if x is None else (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)) for x in models]
            if any(r.shape != (3, 3) for r in rows):
                raise ValueError("a model matrix must be (3, 3)")
            m = torch.from_numpy(np.stack(rows).astype(np.float32)).to(dev)
        if m.numel() != 9 * N:
            raise ValueError(f"model matrices must be ({N}, 3, 3)")
        return m.reshape(N, 9).contiguous()

    def _opts(self, model: Optional[torch.Tensor]):
        """-> the dyb_render_opts of a call (kept alive by the caller) and its address, None when the call is a plain one."""
        if model is None and not self.wireframe:
            return None, None
        o = RenderOpts(model.data_ptr() if model is not None else None, 1 if self.wireframe else 0)
        return o, ctypes.addressof(o)

    def rasterize(self, verts, cam, img=None, color: Sequence[float] = DEFAULT_COLOR, return_normals=False, model=None):
        """-> (image uint8 (N, H, W, 3), face_id int32 (N, H, W), -1 where nothing is drawn, depth fp32 (N, H, W), +inf there);
        without the leading N for a single mesh.  Torch tensors on the inputs' device, or numpy arrays for numpy inputs.
        ``return_normals`` (a debug output) appends the call's vertex normals (N, V, 3), copied out of the workspace.
        ``model``: a (3, 3) matrix, or (N, 3, 3) for a batch, applied to the mesh in the rasteriser's raw model space before it is
        drawn (``side_view_matrix``); the result equals drawing the vertices dyb_render_transform_verts gives, byte for byte."""
        as_numpy = not torch.is_tensor(verts)
        dev = self._device_of(verts, cam, img)
        v = torch.as_tensor(verts, dtype=torch.float32, device=dev) if as_numpy else verts.detach().to(dev, torch.float32)
        c = torch.as_tensor(np.asarray(cam) if not torch.is_tensor(cam) else cam.detach()).to(dev, torch.float32)
        single = v.dim() == 2
        if single:
            v, c = v[None], c.reshape(1, -1)
        if v.dim() != 3 or v.shape[2] != 3 or c.shape != (v.shape[0], 4):
            raise ValueError("verts must be (N, V, 3) or (V, 3) and cam (N, 4) or (4,) = (sx, sy, tx, ty)")
        v, c = v.contiguous(), c.contiguous()
        N, V = int(v.shape[0]), int(v.shape[1])
        W, H = self.resolution
        faces, ptr, idx = self._adjacency(V, dev)
        F = int(faces.shape[0])
        bg = None
        if img is not None:
            bg = torch.as_tensor(img).to(dev)
            if bg.dtype != torch.uint8:
                raise ValueError("the frame under the mesh must be uint8 RGB")
            if single and bg.dim() == 3:
                bg = bg[None]
            if tuple(bg.shape) != (N, H, W, 3):
                raise ValueError(f"frame shape {tuple(bg.shape)} does not match (N, H, W, 3) = {(N, H, W, 3)}")
            bg = bg.contiguous()
        lib = _lib.load()
        if model is not None and not torch.is_tensor(model):
            model = np.asarray(model, np.float32)
            model = [model] if model.ndim == 2 else list(model)
        mats = self._models(model, N, dev)
        opts, optp = self._opts(mats)
        ws = self._workspace(dev, int(lib.dyb_render_workspace_bytes(N, V, F))
                             + (int(lib.dyb_render_model_workspace_bytes(N, V)) if mats is not None else 0))
        out = torch.empty(N, H, W, 3, dtype=torch.uint8, device=dev)
        fid = torch.empty(N, H, W, dtype=torch.int32, device=dev)
        depth = torch.empty(N, H, W, dtype=torch.float32, device=dev)
        col = [float(x) for x in color]
        args = (v.data_ptr(), faces.data_ptr(), ptr.data_ptr(), idx.data_ptr(), c.data_ptr(), bg.data_ptr() if bg is not None else None,
                col[0], col[1], col[2], out.data_ptr(), fid.data_ptr(), depth.data_ptr(), N, V, F, H, W, ws.data_ptr(), ws.numel(),
                stream_of(v))
        # a plain call goes to the plain entry (which forwards to the _opt one with NULL)
        check(lib.dyb_render_meshes(*args) if optp is None else lib.dyb_render_meshes_opt(*args, optp), "dyb_render_meshes")
        res = (out, fid, depth)
        if return_normals:
            res += (ws[:N * V * 12].view(torch.float32).view(N, V, 3).clone(),)
        if single:
            res = tuple(r[0] for r in res)
        if as_numpy:
            res = tuple(r.cpu().numpy() for r in res)
        return res

    def render_many(self, frames, verts_rows, cams, color: Sequence[float] = DEFAULT_COLOR, box: bool = True, models=None):
        """Up to 64 meshes, each over a frame of its own size, in ONE ragged launch (dyb_render_meshes_var).  frames[i]: uint8 RGB
        (H_i, W_i, 3) on the device or None (black - then `resolution` is the size); verts_rows[i]: (V, 3) fp32 on the device - the
        rows may be views into different buffers (result-ring rows of different replicas); cams: (N, 4) = (sx, sy, tx, ty).
        -> list of uint8 (H_i, W_i, 3) tensors, each equal byte for byte to ``render(frames[i], verts_rows[i], cams[i])`` on a
        renderer of that size.  box = False leaves the per-mesh pixel box out (every tile streams the face list; same bytes).
        models: one (3, 3) matrix or None per mesh (or an (N, 3, 3) tensor), as ``render(..., angle, axis)`` applies it."""
        N = len(verts_rows)
        if N == 0:
            return []
        if N > MAX_MESHES or len(frames) != N:
            raise ValueError(f"render_many draws 1 .. {MAX_MESHES} meshes, one frame (or None) each")
        dev = verts_rows[0].device
        c = torch.as_tensor(cams).detach().to(dev, torch.float32).reshape(N, 4).contiguous()
        V = int(verts_rows[0].shape[0])
        faces, ptr, idx = self._adjacency(V, dev)
        F = int(faces.shape[0])
        desc = (RenderDesc * N)()
        keep, outs = [], []
        for i in range(N):
            v = self._row(verts_rows[i], V, dev, "verts_rows must be (V, 3) each, with one V")
            bg, H, W = self._frame(frames[i], dev, "mesh")
            out = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
            desc[i] = RenderDesc(v.data_ptr(), bg.data_ptr() if bg is not None else None, out.data_ptr(), H, W)
            keep += [v, bg]
            outs.append(out)
        lib = _lib.load()
        mats = self._models(models, N, dev)
        opts, optp = self._opts(mats)
        ws = self._workspace(dev, int(lib.dyb_render_var_workspace_bytes(N, V, F))
                             + (int(lib.dyb_render_model_workspace_bytes(N, V)) if mats is not None else 0))
        col = [float(x) for x in color]
        args = (ctypes.cast(desc, ctypes.c_void_p), faces.data_ptr(), ptr.data_ptr(), idx.data_ptr(), c.data_ptr(), col[0], col[1], col[2],
                N, V, F, 0 if box else 1, ws.data_ptr(), ws.numel(), stream_of(c))
        check(lib.dyb_render_meshes_var(*args) if optp is None else lib.dyb_render_meshes_var_opt(*args, optp), "dyb_render_meshes_var")
        return outs

    def render_scenes(self, frames, scenes, return_ids: bool = False):
        """Scenes: several meshes over ONE frame each (all tracked people of a video frame), drawn by dyb_render_scenes.  frames[k]:
        uint8 RGB (H, W, 3) on the device or None (black at `resolution`); scenes[k]: a list of (verts (V, 3), cam (4,) = (sx, sy, tx,
        ty), color (3,)) in painter order - there is no depth test between meshes (each has its own camera, their Z are not
        comparable): the LAST listed mesh is on top wherever it covers a pixel.  A scene may be empty.  An item may carry a fourth
        member, the mesh's (3, 3) model matrix (``side_view_matrix``).
        -> list of uint8 (H, W, 3) tensors, scene k equal byte for byte to the chain  img = frames[k]; for v, c, col in scenes[k]:
        img = render(img, v, c, color=col)  on a renderer of that size.  return_ids: -> (pictures, mesh_ids, face_ids), int32 (H, W)
        each: the winning mesh's position in scenes[k] and its face, -1 where nothing is drawn.
        One call draws at most 64 scenes and 64 meshes; more are packed into several calls, a scene never split - a scene of more
        than 64 meshes is a ValueError."""
        K = len(scenes)
        if len(frames) != K:
            raise ValueError("render_scenes takes one frame (or None) per scene")
        for sc in scenes:
            if len(sc) > MAX_MESHES:
                raise ValueError(f"a scene holds at most {MAX_MESHES} meshes, not {len(sc)}")
        pics, mids, fids = [], [], []
        lo = 0
        while lo < K:
            hi, nm = lo, 0
            while hi < K and hi - lo < MAX_MESHES and nm + len(scenes[hi]) <= MAX_MESHES:
                nm += len(scenes[hi])
                hi += 1
            p, m, f = self._scene_call(frames[lo:hi], scenes[lo:hi], return_ids)
            pics += p
            mids += m
            fids += f
            lo = hi
        return (pics, mids, fids) if return_ids else pics

    def _scene_call(self, frames, scenes, ids):
        meshes = [m for sc in scenes for m in sc]
        dev = self._device_of(*frames, *(m[0] for m in meshes))
        M = len(meshes)
        V = int(meshes[0][0].shape[0]) if M else self.min_verts
        faces, ptr, idx = self._adjacency(V, dev)
        F = int(faces.shape[0])
        desc = (RenderScene * len(scenes))()
        vptr, mscene = (ctypes.c_void_p * max(M, 1))(), (ctypes.c_int * max(M, 1))()
        keep, pics, mids, fids, cams, cols, mods = [], [], [], [], [], [], []
        at = 0
        for k, (bg, sc) in enumerate(zip(frames, scenes)):
            bg, H, W = self._frame(bg, dev, "meshes")
            out = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
            mid = torch.empty(H, W, dtype=torch.int32, device=dev) if ids else None
            fid = torch.empty(H, W, dtype=torch.int32, device=dev) if ids else None
            for item in sc:
                v, cam, col = item[:3]
                mods.append(item[3] if len(item) > 3 else None)
                v = self._row(v, V, dev, "the meshes of a call must be (V, 3) each, with one V")
                vptr[at], mscene[at] = v.data_ptr(), k
                keep.append(v)
                cams.append(torch.as_tensor(cam).detach().to(dev, torch.float32).reshape(4))
                cols.append([float(x) for x in col])
                at += 1
            desc[k] = RenderScene(bg.data_ptr() if bg is not None else None, out.data_ptr(), mid.data_ptr() if ids else None,
                                  fid.data_ptr() if ids else None, H, W, at - len(sc), at)
            keep.append(bg)
            pics.append(out)
            if ids:
                mids.append(mid)
                fids.append(fid)
        cam = torch.stack(cams).contiguous() if M else None
        colors = torch.tensor(cols, dtype=torch.float32).reshape(M, 3).to(dev) if M else None
        lib = _lib.load()
        mats = self._models(mods, M, dev) if M else None
        opts, optp = self._opts(mats)
        ws = self._workspace(dev, int(lib.dyb_render_scenes_workspace_bytes(M, V, F))
                             + (int(lib.dyb_render_model_workspace_bytes(M, V)) if mats is not None else 0))
        args = (ctypes.cast(desc, ctypes.c_void_p), len(scenes), ctypes.cast(vptr, ctypes.c_void_p), ctypes.cast(mscene, ctypes.c_void_p),
                cam.data_ptr() if M else None, colors.data_ptr() if M else None, faces.data_ptr(), ptr.data_ptr(), idx.data_ptr(), M, V, F, 0,
                ws.data_ptr(), ws.numel(), stream_of(ws))
        check(lib.dyb_render_scenes(*args) if optp is None else lib.dyb_render_scenes_opt(*args, optp), "dyb_render_scenes")
        return pics, mids, fids

    def render_scene(self, frame, verts_list, cams, colors=None):
        """One scene: the meshes verts_list[i] (V, 3) under cams[i] = (sx, sy, tx, ty), in painter order (the last on top), over
        `frame` (uint8 (H, W, 3) or None).  colors: one (r, g, b) per mesh; None gives every mesh DEFAULT_COLOR.  -> uint8 (H, W, 3)."""
        n = len(verts_list)
        if len(cams) != n or (colors is not None and len(colors) != n):
            raise ValueError("render_scene takes one camera (and one colour) per mesh")
        cols = [DEFAULT_COLOR] * n if colors is None else colors
        return self.render_scenes([frame], [[(verts_list[i], cams[i], cols[i]) for i in range(n)]])[0]

    def render(self, img, verts, cam, angle=None, axis=None, mesh_filename=None, color: Sequence[float] = DEFAULT_COLOR):
        """The mesh (or batch of meshes) drawn over ``img`` (uint8 RGB, (H, W, 3) or (N, H, W, 3); None = black), as uint8 of the
        kind ``verts`` came in.  ``cam`` = (sx, sy, tx, ty).  As in the reference (render_demo.py:86-98): ``mesh_filename`` writes the
        mesh turned by Rx, (X, -Y, -Z), as a Wavefront .obj - before the side view is applied, one mesh only - and with ``angle``
        (degrees) and ``axis`` both truthy the mesh is turned about the axis before it is drawn; the camera's shift comes after the
        turn."""
        single = (verts.dim() if torch.is_tensor(verts) else np.ndim(verts)) == 2
        if mesh_filename is not None:
            if not single:
                raise ValueError("mesh_filename takes a single mesh (V, 3), not a batch")
            write_obj(mesh_filename, turned_vertices(verts), self.faces)
        turn = bool(angle) and axis is not None and (hasattr(axis, "shape") or bool(axis))
        model = None
        if turn:
            m = side_view_matrix(angle, axis)
            model = m if single else np.broadcast_to(m, (len(verts), 3, 3))
        return self.rasterize(verts, cam, img, color, model=model)[0]
