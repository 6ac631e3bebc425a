"""Numpy restatement of the side-view matrix and the wireframe rule of the mesh overlay (dynaboa_amd/csrc/render.hip, header comment),
on top of tests/render_ref.py: the same snapped coordinates, the same integer coverage, and on the covered centres the wire rule
in exact integers.  Written from the rules, not from the kernel; it shares no code with dynaboa_amd."""
import math

import numpy as np

import render_ref as RR


def rotation(angle_deg, axis):
    """Right-handed rotation by angle_deg about axis, float64 (3, 3): cos I + sin [k]x + (1 - cos) k k^T, the form the reference's
    trimesh.transformations.rotation_matrix evaluates."""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    a = math.radians(angle_deg)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return math.cos(a) * np.eye(3) + math.sin(a) * K + (1.0 - math.cos(a)) * np.outer(k, k)


def side_matrix(angle_deg, axis):
    """What the rasteriser is handed for the reference's side view: Rx R Rx in float64, rounded once to fp32."""
    Rx = np.diag([1.0, -1.0, -1.0])
    return (Rx @ rotation(angle_deg, axis) @ Rx).astype(np.float32)


def transform_bound(m32, verts):
    """-> (exact product in float64 of the fp32 matrix and the fp32 vertices (V, 3), per-component bound 4 * 2^-24 * sum_i |m_i| |v_i|)."""
    m, v = np.asarray(m32, np.float32).astype(np.float64), np.asarray(verts, np.float32).astype(np.float64)
    return v @ m.T, 4.0 * 2.0 ** -24 * (np.abs(v) @ np.abs(m).T)


def _reach(a, b):
    """256 max(|dx|, |dy|) of the edge a -> b, Python integers."""
    return 256 * max(abs(int(b[0]) - int(a[0])), abs(int(b[1]) - int(a[1])))


def wire_mask(xy, face, px, py):
    """-> (fragment bool array, weights, area): the centres (px, py) inside `face` by the coverage rule AND within one pixel, along the
    minor axis, of one of its edges: w_e < 256 max(|dx_e|, |dy_e|)."""
    inside, w, area = RR.face_weights(xy, face, px, py)
    if area <= 0:
        return inside, w, area
    p0, p1, p2 = (tuple(int(c) for c in xy[i]) for i in face)
    a, b, c = p0, p2, p1                          # render_ref's drawn orientation; w = (w of v0, v1, v2) = (wa, wc, wb)
    wa, wc, wb = w
    near = np.zeros(np.shape(px), bool)
    for we, (e0, e1) in ((wa, (b, c)), (wb, (c, a)), (wc, (a, b))):      # the weight of a corner is the edge function of the edge opposite
        r = _reach(e0, e1)                        # a Python integer, at most 256 * 2^31: exact as int64 beside render_ref's int64 weights
        near |= we < np.int64(r)
    return inside & near, w, area


def shade32(verts, faces, normals, face_id, w, area, background, color):
    """The shading rule of the header comment in fp32, one rounding per operation in the order the rule is written (sums left to
    right), for the pixels where face_id >= 0: barycentric weights = the integer weights converted to fp32 over the converted area,
    normal and position interpolated, normal renormalised, both taken to the turned space (x, -y, -z), the three lights, ambient
    0.3, pixel = round(255 I colour).  `normals`: the fp32 vertex normals (V, 3) - the caller's, as their own sum order is not part
    of this rule.  IEEE arithmetic (division and square root correctly rounded): numpy's float32 gives the device's bits."""
    f32 = np.float32
    P, N = np.asarray(verts, f32), np.asarray(normals, f32)
    H, W = face_id.shape
    img = np.zeros((H, W, 3), np.uint8) if background is None else np.array(background, np.uint8)
    cov = face_id >= 0
    tri = np.asarray(faces, np.int64)[face_id[cov]]
    ar = area[cov].astype(f32)
    b = [w[k][cov].astype(f32) / ar for k in range(3)]

    def mix(A, c):
        return (b[0] * A[tri[:, 0], c] + b[1] * A[tri[:, 1], c]) + b[2] * A[tri[:, 2], c]
    nx, ny, nz = mix(N, 0), mix(N, 1), mix(N, 2)
    nl = np.sqrt((nx * nx + ny * ny) + nz * nz)
    with np.errstate(all="ignore"):
        ni = np.where(nl > 0, f32(1.0) / nl, f32(0.0)).astype(f32)
    nx, ny, nz = nx * ni, -(ny * ni), -(nz * ni)
    qx, qy, qz = mix(P, 0), -mix(P, 1), -mix(P, 2)
    total = np.zeros(len(ar), f32)
    for L in RR.LIGHTS.astype(f32):
        dx, dy, dz = L[0] - qx, L[1] - qy, L[2] - qz
        dl = np.sqrt((dx * dx + dy * dy) + dz * dz)
        with np.errstate(all="ignore"):
            dot = np.where(dl > 0, ((nx * dx + ny * dy) + nz * dz) / dl, f32(0.0)).astype(f32)
        total = total + np.maximum(dot, f32(0.0))
    I = np.minimum(f32(0.3) + f32(0.35) * total, f32(1.0))
    col = np.asarray(color, np.float64).astype(f32)
    img[cov] = np.stack([np.clip(np.rint((f32(255.0) * I) * col[k]), 0, 255) for k in range(3)], 1).astype(np.uint8)
    return img


def render_wire(verts, faces, cam, H, W, background=None, color=(1.0, 1.0, 0.9), normals=None):
    """One mesh as wireframe -> render_ref.Result (face_id, depth float64, image): nearest fragment wins, ties to the lower face index,
    depth as render_ref.render gives it for the solid mesh.  image: the shading in float64 as render_ref.render states it (from its
    own vertex normals); with `normals` (fp32 (V, 3)) also image32, the same rule in fp32 (shade32)."""
    faces = np.asarray(faces, np.int64)
    xy, ok = RR.snap(verts, cam, H, W)
    R = RR.Result(H, W, verts, faces, xy, ok)
    v64 = R.verts
    wi = np.zeros((3, H, W), np.int64)
    ai = np.ones((H, W), np.int64)
    for f, face in enumerate(faces):
        if not ok[face].all():
            continue
        p = xy[face]
        ilo, ihi = max(int(-(-(p[:, 0].min() - 128) // 256)), 0), min(int((p[:, 0].max() - 128) // 256), W - 1)
        jlo, jhi = max(int(-(-(p[:, 1].min() - 128) // 256)), 0), min(int((p[:, 1].max() - 128) // 256), H - 1)
        if ilo > ihi or jlo > jhi:
            continue
        py, px = np.meshgrid(256 * np.arange(jlo, jhi + 1, dtype=np.int64) + 128, 256 * np.arange(ilo, ihi + 1, dtype=np.int64) + 128,
                             indexing="ij")
        frag, w, area = wire_mask(xy, face, px, py)
        if not frag.any():
            continue
        z = v64[face, 2]
        d = (w[0].astype(np.float64) * z[0] + w[1].astype(np.float64) * z[1] + w[2].astype(np.float64) * z[2]) / float(area)
        sub = (slice(jlo, jhi + 1), slice(ilo, ihi + 1))
        win = frag & (d < R.depth[sub])
        R.depth[sub][win] = d[win]
        R.face_id[sub][win] = f
        for k in range(3):
            wi[k][sub][win] = w[k][win]
        ai[sub][win] = area
    R.weights, R.area = wi, ai
    # the solid path's shading, restated as render_ref.render states it
    vn = RR.vertex_normals(verts, faces)
    img = np.zeros((H, W, 3), np.uint8) if background is None else np.array(background, np.uint8)
    cov = R.face_id >= 0
    fsel = faces[R.face_id[cov]]
    b = np.stack([wi[k][cov].astype(np.float64) / ai[cov].astype(np.float64) for k in range(3)], 1)
    n = (b[:, :, None] * vn[fsel]).sum(1)
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    n = np.divide(n, ln, out=np.zeros_like(n), where=ln > 0)
    q = (b[:, :, None] * v64[fsel]).sum(1)
    flip = np.array([1.0, -1.0, -1.0])
    n, q = n * flip, q * flip
    total = np.zeros(len(q))
    for L in RR.LIGHTS:
        d = L[None] - q
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        total += np.maximum((n * d).sum(1), 0.0)
    I = np.minimum(0.3 + 0.35 * total, 1.0)
    col = np.asarray(color, np.float32).astype(np.float64)
    img[cov] = np.clip(np.rint(255.0 * I[:, None] * col[None]), 0, 255).astype(np.uint8)
    R.image = img
    R.vertex_normals = vn
    R.image32 = None if normals is None else shade32(verts, faces, normals, R.face_id, wi, ai, background, color)
    return R


def parse_obj(path):
    """-> (vertices fp32 (V, 3), faces int64 (F, 3) as written: 1-based) of a Wavefront file of ``v`` and ``f`` lines only."""
    vs, fs = [], []
    for line in open(path).read().splitlines():
        t = line.split()
        assert t and t[0] in ("v", "f") and len(t) == 4, line
        if t[0] == "v":
            assert not fs, "vertices come before faces"
            vs.append([np.float32(x) for x in t[1:]])
        else:
            fs.append([int(x) for x in t[1:]])
    return np.array(vs, np.float32).reshape(-1, 3), np.array(fs, np.int64).reshape(-1, 3)
