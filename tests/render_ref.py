"""Plain numpy restatement of the mesh overlay's rules (dynaboa_amd/csrc/render.hip, header comment), one face at a time:
fp32 image positions snapped to 1/256 pixel exactly as the kernel forms them, int64 coverage with the top-left rule, float64
depth and shading.  Written from the rules, not from the kernel; it shares no code with dynaboa_amd."""
import numpy as np

LIGHTS = np.array([[0.0, -1.0, 1.0], [0.0, 1.0, 1.0], [1.0, 1.0, 2.0]])
SNAP_LIMIT = np.float32(2.0 ** 30)


def snap(verts, cam, H, W):
    """-> (xy int64 (V, 2) in 1/256 pixel, ok (V,)): fp32 arithmetic, one rounding per operation, round half to even."""
    v = np.asarray(verts, np.float32)
    sx, sy, tx, ty = (np.float32(c) for c in cam)
    one, hw, hh, s = np.float32(1.0), np.float32(0.5) * np.float32(W), np.float32(0.5) * np.float32(H), np.float32(256.0)
    with np.errstate(all="ignore"):
        fu = np.rint((hw * (one + sx * (v[:, 0] + tx))) * s)
        fv = np.rint((hh * (one + sy * (v[:, 1] + ty))) * s)
        ok = (np.abs(fu) <= SNAP_LIMIT) & (np.abs(fv) <= SNAP_LIMIT) & np.isfinite(v[:, 2])       # a face needs finite depths
    xy = np.stack([np.where(ok, fu, 0), np.where(ok, fv, 0)], 1).astype(np.int64)
    return xy, ok


def _edge(a, b, px, py):
    return (b[0] - a[0]) * (py - a[1]) - (b[1] - a[1]) * (px - a[0])


def _owns(a, b):
    """Top-left rule for edge a -> b of a triangle with positive area in (x right, y down) under _edge: left edges run up,
    top edges run right."""
    return b[1] < a[1] or (b[1] == a[1] and b[0] > a[0])


def face_weights(xy, face, px, py):
    """Integer coverage of pixel centres (px, py) (1/256-pixel units, arrays) by `face` = (i0, i1, i2).
    -> (inside bool, (w0, w1, w2) int64 weights of the three vertices, area int64); area <= 0 = culled (inside all False)."""
    p0, p1, p2 = (tuple(int(c) for c in xy[i]) for i in face)
    a, b, c = p0, p2, p1                        # the drawn orientation: front faces (model normal Z < 0) have positive area
    area = _edge(a, b, c[0], c[1])
    wa, wb, wc = _edge(b, c, px, py), _edge(c, a, px, py), _edge(a, b, px, py)
    if area <= 0:
        return np.zeros(np.shape(px), bool), (wa, wc, wb), area
    inside = ((wa - (0 if _owns(b, c) else 1)) >= 0) & ((wb - (0 if _owns(c, a) else 1)) >= 0) & ((wc - (0 if _owns(a, b) else 1)) >= 0)
    return inside, (wa, wc, wb), area


def vertex_normals(verts, faces):
    """Normalised sum of the unnormalised normals of the incident faces (float64); zero where the sum vanishes."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    vn = np.zeros_like(v)
    for k in range(3):
        np.add.at(vn, f[:, k], fn)
    ln = np.linalg.norm(vn, axis=1, keepdims=True)
    return np.divide(vn, ln, out=np.zeros_like(vn), where=ln > 0)


class Result:
    def __init__(self, H, W, verts, faces, xy, ok):
        self.H, self.W, self.verts, self.faces, self.xy, self.ok = H, W, np.asarray(verts, np.float64), faces, xy, ok
        self.face_id = np.full((H, W), -1, np.int32)
        self.depth = np.full((H, W), np.inf)
        self.image = None
        self.covering = None                    # [(j, i)] -> list of (face, depth) when asked for

    def covers(self, j, i, f):
        """(inside by the integer test, float64 depth) of face f at pixel (row j, column i)."""
        face = self.faces[f]
        if not self.ok[face].all():
            return False, np.inf
        inside, w, area = face_weights(self.xy, face, np.int64(256 * i + 128), np.int64(256 * j + 128))
        if not bool(inside):
            return False, np.inf
        z = self.verts[face, 2]
        return True, (float(w[0]) * z[0] + float(w[1]) * z[1] + float(w[2]) * z[2]) / float(area)


def render(verts, faces, cam, H, W, background=None, color=(1.0, 1.0, 0.9), keep_covering=False):
    """One mesh.  -> Result with face_id (H, W) int32 (-1 = nothing), depth (H, W) float64 (+inf = nothing), image (H, W, 3)
    uint8 and, with keep_covering, covering[(j, i)] = [(face, depth), ...] in face order."""
    faces = np.asarray(faces, np.int64)
    xy, ok = snap(verts, cam, H, W)
    R = Result(H, W, verts, faces, xy, ok)
    v64 = R.verts
    w_best = np.zeros((3, H, W))
    if keep_covering:
        R.covering = {}
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
        inside, w, area = face_weights(xy, face, px, py)
        if not inside.any():
            continue
        z = v64[face, 2]
        d = (w[0].astype(np.float64) * z[0] + w[1].astype(np.float64) * z[1] + w[2].astype(np.float64) * z[2]) / float(area)
        sub = (slice(jlo, jhi + 1), slice(ilo, ihi + 1))
        if keep_covering:
            for jj, ii in zip(*np.nonzero(inside)):
                R.covering.setdefault((jlo + int(jj), ilo + int(ii)), []).append((f, float(d[jj, ii])))
        win = inside & (d < R.depth[sub])        # faces come in ascending order: a tie keeps the lower index
        R.depth[sub][win] = d[win]
        R.face_id[sub][win] = f
        for k in range(3):
            w_best[k][sub][win] = w[k][win].astype(np.float64) / float(area)
    # smooth shading in the turned space (x, -y, -z)
    vn = vertex_normals(verts, faces)
    img = np.zeros((H, W, 3), np.uint8) if background is None else np.array(background, np.uint8)
    cov = R.face_id >= 0
    fsel = faces[R.face_id[cov]]
    b = np.stack([w_best[k][cov] for k in range(3)], 1)
    n = (b[:, :, None] * vn[fsel]).sum(1)
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    n = np.divide(n, ln, out=np.zeros_like(n), where=ln > 0)
    q = (b[:, :, None] * v64[fsel]).sum(1)
    flip = np.array([1.0, -1.0, -1.0])
    n, q = n * flip, q * flip
    total = np.zeros(len(q))
    for L in LIGHTS:
        d = L[None] - q
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        total += np.maximum((n * d).sum(1), 0.0)
    I = np.minimum(0.3 + 0.35 * total, 1.0)
    col = np.asarray(color, np.float32).astype(np.float64)
    img[cov] = np.clip(np.rint(255.0 * I[:, None] * col[None]), 0, 255).astype(np.uint8)
    R.image = img
    R.shade = np.zeros((H, W))
    R.shade[cov] = I
    R.vertex_normals = vn
    return R
