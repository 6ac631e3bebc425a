"""Backend-agnostic checks of dyb_smooth_sequences and dyb_one_euro_step (csrc/smooth.hip): each takes a backend of tests/backends.py,
so the same cases run on the kernel emulator and on the device.  The reference has no smoother; the oracle is the restatement below of
the rules of include/dynaboa_hip.h in NumPy, evaluated in float64 (and in float32, for the tolerance).

Inputs (seeded): per joint a slow axis-angle sinusoid (amplitude 0.2 - 0.8 rad, 0.005 - 0.02 cycles per frame) plus Gaussian noise of
0.05 rad; joint 0 instead swings by +-0.3 rad about (3.0, 0, 0), across the angle pi.  That alone does not flip a sign: about pi
around +x rot_to_quat stays in the branch that makes the x component positive, and w passes through zero continuously (measured: no
negative dot product between neighbours).  So joint 1 swings by +-0.3 rad about (-pi / 2, 0, 0): there r22 = cos(angle) crosses the
formula's threshold, the branch changes between "w positive" and "x positive" while x is negative, and the result changes sign
between neighbouring frames.  Sequence lengths 1, 2, 3, 7, 40, 0, 25 (78 frames), J = 24, nb = 10, nc = 3.  The
kernel has no frame tile: a workgroup owns 256 consecutive (frame, group) elements, 10.24 frames at J = 24, so the 40-frame and the
25-frame run (frames 53 .. 77, which would also straddle a 64-frame tile) cross several workgroup boundaries with taps on both sides.

Two conditions on the inputs, asserted by a CPU test: for every (centre, tap) pair within 8 frames of one run |dot(q_tap, q_centre)|
>= 0.5, so no rounding can decide a sign (SIGN_MARGIN; measured 0.90); and at least one adjacent pair has a negative dot product.

Tolerance.  The restatement is evaluated in float32 and in float64 on these inputs (h = 1, 4, 8, 32; the One-Euro stream); the bound
is 8 x the largest difference - room for FMA contraction and a reciprocal square root against sqrt and divide.
  window:   measured floor 7.11e-7 -> FLOOR 7.2e-7, BOUND 5.76e-6
  One-Euro: measured floor 4.20e-7 -> OE_FLOOR 4.3e-7, OE_BOUND 3.44e-6
test_smooth_kernels.py::test_measured_floors asserts that the measured floors lie in (FLOOR / 2, FLOOR]."""
import numpy as np

LENGTHS = (1, 2, 3, 7, 40, 0, 25)
J, NB, NC = 24, 10, 3
SENTINEL = 123.5
ERR_ARG = -1
SIGN_MARGIN = 0.5
FLOOR, OE_FLOOR = 7.2e-7, 4.3e-7
BOUND, OE_BOUND = 8 * FLOOR, 8 * OE_FLOOR
EPS32 = float(np.float32(1e-6))
MIN_NORM2 = float(np.float32(1e-12))


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------ the inputs
def rodrigues(aa):
    """axis-angle (..., 3) float64 -> rotation matrices (..., 9)."""
    th = np.linalg.norm(aa, axis=-1, keepdims=True)
    k = aa / np.maximum(th, 1e-12)
    x, y, z = k[..., 0], k[..., 1], k[..., 2]
    c, s = np.cos(th[..., 0]), np.sin(th[..., 0])
    C = 1 - c
    return np.stack([c + x * x * C, x * y * C - z * s, x * z * C + y * s, y * x * C + z * s, c + y * y * C, y * z * C - x * s,
                     z * x * C - y * s, z * y * C + x * s, c + z * z * C], -1)


def make_inputs(lengths=LENGTHS, J=J, nb=NB, nc=NC, seed=2024):
    """-> dict: rotmat [n][J][9], betas [n][nb], cam [n][nc] fp32 (noisy), clean_rotmat (fp64, the trajectory without noise) and
    clean_aa [n][J][3], its axis-angle form."""
    rng = np.random.default_rng(seed)
    rot, clean, betas, cam, aa_clean = [], [], [], [], []
    for n in lengths:
        t = np.arange(n)[:, None, None]
        amp, freq = rng.uniform(0.2, 0.8, (1, J, 3)), rng.uniform(0.005, 0.02, (1, J, 3))
        aa = amp * np.sin(2 * np.pi * freq * t + rng.uniform(0, 6, (1, J, 3)))
        aa[:, 0] = np.array([3.0, 0, 0]) + 0.3 * np.sin(2 * np.pi * 0.02 * t[:, 0] + rng.uniform(0, 6, (1, 3)))
        if J > 1:
            aa[:, 1] = np.array([-np.pi / 2, 0, 0]) + 0.3 * np.sin(2 * np.pi * 0.02 * t[:, 0] + rng.uniform(0, 6, (1, 3)))
        clean.append(rodrigues(aa))
        aa_clean.append(aa)
        rot.append(rodrigues(aa + rng.normal(0, 0.05, aa.shape)))
        tt = np.arange(n)[:, None]
        betas.append(rng.normal(0, 1, (1, nb)) + 0.3 * np.sin(0.05 * tt + rng.uniform(0, 6, (1, nb))) + rng.normal(0, 0.05, (n, nb)))
        cam.append(np.array([[0.9] + [0.0] * (nc - 1)]) + 0.1 * np.sin(0.04 * tt + rng.uniform(0, 6, (1, nc))) + rng.normal(0, 0.01, (n, nc)))
    f = lambda parts, w: np.concatenate(parts).reshape(sum(lengths), *w)
    return dict(rotmat=f(rot, (J, 9)).astype(np.float32), clean_rotmat=f(clean, (J, 9)), betas=f(betas, (nb,)).astype(np.float32),
                cam=f(cam, (nc,)).astype(np.float32), clean_aa=f(aa_clean, (J, 3)))


def gaussian(h, sigma=None):
    """The weights of dynaboa_amd.smooth.gaussian_weights, restated."""
    sigma = h / 2.0 if sigma is None else sigma
    k = np.arange(-h, h + 1, dtype=np.float64)
    return np.exp(-0.5 * (k / sigma) ** 2).astype(np.float32) if h > 0 else np.ones(1, np.float32)


# ------------------------------------------------------------------------------------------------------------------ the restatement
def rot_to_quat(R, dt):
    """csrc/dyb_quat.h: the four-branch formula on (..., 9) matrices, arithmetic in `dt`; -> (..., 4) = (w, x, y, z)."""
    R = np.asarray(R, dt)
    r00, r01, r02, r10, r11, r12, r20, r21, r22 = (R[..., i] for i in range(9))
    one = dt(1)
    d2, d01, d0n1 = r22 < dt(EPS32), r00 > r11, r00 < -r11
    b0, b1, b2 = d2 & d01, d2 & ~d01, ~d2 & d0n1
    t0, t1, t2, t3 = one + r00 - r11 - r22, one - r00 + r11 - r22, one - r00 - r11 + r22, one + r00 + r11 + r22
    u0 = np.stack([r21 - r12, t0, r10 + r01, r02 + r20], -1)
    u1 = np.stack([r02 - r20, r10 + r01, t1, r21 + r12], -1)
    u2 = np.stack([r10 - r01, r02 + r20, r21 + r12, t2], -1)
    u3 = np.stack([t3, r21 - r12, r02 - r20, r10 - r01], -1)
    u = np.where(b0[..., None], u0, np.where(b1[..., None], u1, np.where(b2[..., None], u2, u3)))
    t = np.where(b0, t0, np.where(b1, t1, np.where(b2, t2, t3)))
    with np.errstate(invalid="ignore", divide="ignore"):
        return (u * (dt(0.5) / np.sqrt(t))[..., None]).astype(dt)


def quat_to_rot(q, dt):
    w, x, y, z = (q[..., i] for i in range(4))
    one, two = dt(1), dt(2)
    return np.stack([one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y),
                     two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x),
                     two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)], -1).astype(dt)


def linked(lengths, n, valid=None, frame_id=None):
    """link[i]: frames i and i + 1 are linked."""
    off = offsets_of(lengths)
    seq = np.searchsorted(off, np.arange(n), side="right") - 1
    link = np.zeros(max(n, 1), bool)
    for i in range(n - 1):
        ok = seq[i] == seq[i + 1]
        if ok and valid is not None:
            ok = bool(valid[i]) and bool(valid[i + 1])
        if ok and frame_id is not None:
            ok = int(frame_id[i + 1]) == int(frame_id[i]) + 1
        link[i] = ok
    return link


def window_of(link, i, h, n, valid=None):
    """-> (back, fwd): the taps i - back .. i + fwd of frame i."""
    if h == 0 or (valid is not None and not valid[i]):
        return 0, 0
    back = fwd = 0
    while back < h and i - back - 1 >= 0 and link[i - back - 1]:
        back += 1
    while fwd < h and i + fwd + 1 < n and link[i + fwd]:
        fwd += 1
    return back, fwd


def ref_smooth(rotmat, betas, cam, lengths, weights, h, valid=None, frame_id=None, dt=np.float64):
    """The rules of dyb_smooth_sequences, arithmetic in `dt` -> (rotmat, betas, cam), copies where the kernel copies."""
    n = rotmat.shape[0]
    w = np.asarray(weights, np.float32).astype(dt)
    out = [np.array(rotmat, np.float32).astype(dt), None if betas is None else np.array(betas, np.float32).astype(dt),
           None if cam is None else np.array(cam, np.float32).astype(dt)]
    link = linked(lengths, n, valid, frame_id)
    with np.errstate(invalid="ignore"):
        q_all = rot_to_quat(rotmat, dt)
    for i in range(n):
        back, fwd = window_of(link, i, h, n, valid)
        if back + fwd == 0:
            continue
        qc = q_all[i]
        s = np.zeros_like(qc)
        for k in range(-back, fwd + 1):
            qk = q_all[i + k]
            ok = np.isfinite(qk).all(-1)
            with np.errstate(invalid="ignore"):
                d = ((qk[:, 0] * qc[:, 0] + qk[:, 1] * qc[:, 1]) + qk[:, 2] * qc[:, 2]) + qk[:, 3] * qc[:, 3]
                wk = np.where(d < 0, -w[k + h], w[k + h]).astype(dt)
                s = np.where(ok[:, None], s + wk[:, None] * qk, s).astype(dt)
        n2 = ((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]) + s[:, 3] * s[:, 3]
        good = np.isfinite(qc).all(-1) & (n2 >= dt(MIN_NORM2))
        with np.errstate(invalid="ignore", divide="ignore"):
            R = quat_to_rot(s * (dt(1) / np.sqrt(n2))[:, None], dt)
        out[0][i] = np.where(good[:, None], R, out[0][i])
        for slot, x in ((1, betas), (2, cam)):
            if x is None:
                continue
            x = np.asarray(x, np.float32).astype(dt)
            wsum, acc = dt(0), np.zeros(x.shape[1], dt)
            for k in range(-back, fwd + 1):
                wsum = dt(wsum + w[k + h])
                acc = (acc + w[k + h] * x[i + k]).astype(dt)
            out[slot][i] = acc / wsum
    return out


def ref_one_euro_step(state, rotmat, betas, cam, active, te, min_cutoff, beta, d_cutoff, dt=np.float64):
    """One step of the rules of dyb_one_euro_step on `state` (a dict of dt arrays per sequence: started, xh, dxh), in place;
    -> (rotmat, betas, cam) outputs, NaN rows where the sequence is inactive."""
    R, Jn = rotmat.shape[0], rotmat.shape[1]
    te, min_cutoff, beta, d_cutoff = dt(te), dt(min_cutoff), dt(beta), dt(d_cutoff)
    twopi = dt(np.float32(6.2831853071795864769)) if dt is np.float32 else dt(2 * np.pi)
    alpha = lambda c: dt(1) / (dt(1) + (dt(1) / (twopi * c)) / te)
    outs = [np.full(rotmat.shape, np.nan, dt), np.full(betas.shape, np.nan, dt), np.full(cam.shape, np.nan, dt)]
    a_d = alpha(d_cutoff)
    for r in range(R):
        if active is not None and not active[r]:
            continue
        q = rot_to_quat(rotmat[r], dt)
        x = np.concatenate([q.reshape(-1), betas[r].astype(dt), cam[r].astype(dt)])
        st = state[r]
        if not st["started"]:
            st["started"], st["xh"], st["dxh"] = True, x.copy(), np.zeros_like(x)
            outs[0][r], outs[1][r], outs[2][r] = rotmat[r], betas[r], cam[r]
            continue
        xh, dxh = st["xh"], st["dxh"]
        groups = [slice(4 * j, 4 * j + 4) for j in range(Jn)] + [slice(4 * Jn + c, 4 * Jn + c + 1) for c in range(len(x) - 4 * Jn)]
        for gi, g in enumerate(groups):
            xs = x[g]
            if gi < Jn:
                d = ((xs[0] * xh[g][0] + xs[1] * xh[g][1]) + xs[2] * xh[g][2]) + xs[3] * xh[g][3]
                if d < 0:
                    xs = -xs
            dx = ((xs - xh[g]) / te).astype(dt)
            dxh[g] = (a_d * dx + (dt(1) - a_d) * dxh[g]).astype(dt)
            a = alpha(dt(min_cutoff + beta * np.sqrt(np.sum(dxh[g] * dxh[g], dtype=dt))))
            v = (a * xs + (dt(1) - a) * xh[g]).astype(dt)
            if gi < Jn:
                v = (v * (dt(1) / np.sqrt(np.sum(v * v, dtype=dt)))).astype(dt)
            xh[g] = v
        outs[0][r] = quat_to_rot(xh[:4 * Jn].reshape(Jn, 4), dt)
        outs[1][r], outs[2][r] = xh[4 * Jn:4 * Jn + betas.shape[1]], xh[4 * Jn + betas.shape[1]:]
    return outs


# ------------------------------------------------------------------------------------------------------------------ conditions
def sign_margin(rotmat, lengths, reach=8):
    """-> (the smallest |dot(q_tap, q_centre)| over pairs within `reach` frames of one sequence, the number of adjacent pairs with a
    negative dot product)."""
    q = rot_to_quat(rotmat, np.float64)
    off = offsets_of(lengths)
    low, flips = 1.0, 0
    for a, b in zip(off[:-1], off[1:]):
        for i in range(a, b):
            for k in range(i + 1, min(i + reach, b - 1) + 1):
                d = np.sum(q[i] * q[k], -1)
                low = min(low, float(np.abs(d).min()))
                if k == i + 1:
                    flips += int((d < 0).sum())
    return low, flips


def measure_floor(hs=(1, 4, 8, 32)):
    """The largest difference between the float32 and the float64 evaluation of the restatement on the test's inputs."""
    x = make_inputs()
    worst = 0.0
    for h in hs:
        a = ref_smooth(x["rotmat"], x["betas"], x["cam"], LENGTHS, gaussian(h), h, dt=np.float32)
        b = ref_smooth(x["rotmat"], x["betas"], x["cam"], LENGTHS, gaussian(h), h, dt=np.float64)
        worst = max(worst, *(float(np.abs(p.astype(np.float64) - q).max()) for p, q in zip(a, b)))
    return worst


# ------------------------------------------------------------------------------------------------------------------ the window: driver
def run(be, rotmat, betas, cam, lengths, weights, h, valid=None, frame_id=None, null=(), n=None, n_seq=None, J=None, nb=None, nc=None,
        alias=None):
    """-> (rc, rotmat_out, betas_out, cam_out); the outputs start filled with SENTINEL.  `null`: argument names passed as NULL;
    `alias`: an output name that is given its input's buffer."""
    N, Jn = rotmat.shape[0], rotmat.shape[1]
    w = np.ascontiguousarray(np.asarray(weights, np.float32))           # HOST memory on either backend
    off = offsets_of(lengths)
    sent = lambda x: None if x is None else be.dev(np.full(tuple(max(d, 1) for d in x.shape), SENTINEL, np.float32))
    a = dict(rotmat=be.dev(rotmat), betas=None if betas is None else be.dev(betas), cam=None if cam is None else be.dev(cam),
             off=be.dev(off, np.int32), valid=None if valid is None else be.dev(valid, np.uint8),
             fid=None if frame_id is None else be.dev(frame_id, np.int32), rotmat_out=sent(rotmat), betas_out=sent(betas), cam_out=sent(cam))
    p = {k: (None if k in null else be.ptr(v)) for k, v in a.items()}
    if alias:
        p[alias + "_out"] = p[alias]
    rc = be.lib.dyb_smooth_sequences(p["rotmat"], p["betas"], (0 if betas is None else betas.shape[1]) if nb is None else nb, p["cam"],
                                     (0 if cam is None else cam.shape[1]) if nc is None else nc, p["off"],
                                     len(lengths) if n_seq is None else n_seq, p["valid"], p["fid"],
                                     None if "weights" in null else w.ctypes.data, int(h), p["rotmat_out"], p["betas_out"], p["cam_out"],
                                     N if n is None else n, Jn if J is None else J, be.stream)
    host = lambda x, ref: None if x is None else be.host(x)[:ref.shape[0]]
    return rc, host(a["rotmat_out"], rotmat), host(a["betas_out"], betas), host(a["cam_out"], cam)


def check(got, ref, bound=BOUND):
    for g, r in zip(got, ref):
        if r is None:
            assert g is None
            continue
        err = float(np.abs(g.astype(np.float64) - r).max()) if r.size else 0.0
        assert np.isfinite(g).all() and err <= bound, err


def check_orthonormal(R, bound=BOUND):
    M = R.reshape(-1, 3, 3).astype(np.float64)
    err = np.abs(M @ M.transpose(0, 2, 1) - np.eye(3)).max()
    det = np.abs(np.linalg.det(M) - 1).max()
    assert err <= bound and det <= bound, (err, det)


def case_batch(be, h):
    """The ragged batch against the restatement; h = 32 is a window larger than every run.  Orthonormal outputs, determinant +1."""
    x = make_inputs()
    w = gaussian(h)
    rc, R, B, C = run(be, x["rotmat"], x["betas"], x["cam"], LENGTHS, w, h)
    assert rc == 0
    check((R, B, C), ref_smooth(x["rotmat"], x["betas"], x["cam"], LENGTHS, w, h))
    check_orthonormal(R)
    assert R[0].tobytes() == x["rotmat"][0].tobytes() and B[0].tobytes() == x["betas"][0].tobytes()      # the length-1 sequence
    assert not np.array_equal(R[20], x["rotmat"][20])


def case_channels(be):
    """J = 1; betas NULL; cam NULL; nc = 4."""
    for kw in (dict(J=1), dict(nb=0), dict(nc=0), dict(nc=4), dict(nb=0, nc=0)):
        Jn, nb, nc = kw.get("J", 5), kw.get("nb", 3), kw.get("nc", 3)
        x = make_inputs((3, 12, 1), Jn, max(nb, 1), max(nc, 1), seed=7)
        betas, cam = x["betas"] if nb else None, x["cam"] if nc else None
        w = gaussian(3)
        rc, R, B, C = run(be, x["rotmat"], betas, cam, (3, 12, 1), w, 3)
        assert rc == 0, kw
        check((R, B, C), ref_smooth(x["rotmat"], betas, cam, (3, 12, 1), w, 3))


def case_tile_boundary(be):
    """One sequence of 600 frames at J = 24 (59 workgroups of 256 elements) and frames 53 .. 77 of the standard batch: runs that
    cross workgroup boundaries with taps on both sides; uneven weights, so a tap taken from the wrong side would show."""
    w = np.array([0.1, 0.7, 0.2, 1.0, 2.0, 0.0, 0.4, 0.3, 0.9], np.float32)
    x = make_inputs((600,), seed=11)
    rc, R, B, C = run(be, x["rotmat"], x["betas"], x["cam"], (600,), w, 4)
    assert rc == 0
    check((R, B, C), ref_smooth(x["rotmat"], x["betas"], x["cam"], (600,), w, 4))
    x = make_inputs()
    rc, R, B, C = run(be, x["rotmat"], x["betas"], x["cam"], LENGTHS, w, 4)
    ref = ref_smooth(x["rotmat"], x["betas"], x["cam"], LENGTHS, w, 4)
    check((R[53:78], B[53:78], C[53:78]), [r[53:78] for r in ref])


def case_masks(be):
    """Holes in `valid` and a gap in `frame_id` each split a run; invalid frames are byte copies; a NaN planted in an invalid frame
    reaches no other output."""
    x = make_inputs()
    off = offsets_of(LENGTHS)
    h, w = 4, gaussian(4)
    n = sum(LENGTHS)
    valid = np.ones(n, np.uint8)
    valid[[off[4] + 10, off[4] + 12, off[6] + 3]] = 0                    # frame off[4] + 11 is alone between two invalid ones
    fid = np.concatenate([np.arange(m) + 5 * s for s, m in enumerate(LENGTHS)]).astype(np.int32)
    fid[off[6] + 15:] += 2                                               # a gap inside the 25-frame sequence
    rc, R, B, C = run(be, x["rotmat"], x["betas"], x["cam"], LENGTHS, w, h, valid=valid, frame_id=fid)
    assert rc == 0
    check((R, B, C), ref_smooth(x["rotmat"], x["betas"], x["cam"], LENGTHS, w, h, valid=valid, frame_id=fid))
    for i in (off[4] + 10, off[4] + 11, off[4] + 12, off[6] + 3):
        assert R[i].tobytes() == x["rotmat"][i].tobytes() and B[i].tobytes() == x["betas"][i].tobytes() and C[i].tobytes() == x["cam"][i].tobytes(), i
    # the run 53..67 | 68..77: the output of frame 67 is that of a sequence ending there
    cut = off[6] + 15
    lens2 = list(LENGTHS[:6]) + [15, 10]
    _, R2, B2, C2 = run(be, x["rotmat"], x["betas"], x["cam"], lens2, w, h, valid=valid)
    assert R2.tobytes() == R.tobytes() and B2.tobytes() == B.tobytes() and C2.tobytes() == C.tobytes() and cut == 68
    # consecutive ids change nothing
    _, Ra, _, _ = run(be, x["rotmat"], x["betas"], x["cam"], LENGTHS, w, h)
    _, Rb, _, _ = run(be, x["rotmat"], x["betas"], x["cam"], LENGTHS, w, h, frame_id=np.arange(n).astype(np.int32) + 100)
    assert Ra.tobytes() == Rb.tobytes()
    # NaN in the invalid frames: copied through, every other output finite and equal to the output with those frames zeroed
    bad = np.flatnonzero(valid == 0)
    xn = {k: v.copy() for k, v in x.items()}
    xz = {k: v.copy() for k, v in x.items()}
    for k in ("rotmat", "betas", "cam"):
        xn[k][bad], xz[k][bad] = np.nan, 0.0
    _, Rn, Bn, Cn = run(be, xn["rotmat"], xn["betas"], xn["cam"], LENGTHS, w, h, valid=valid, frame_id=fid)
    _, Rz, Bz, Cz = run(be, xz["rotmat"], xz["betas"], xz["cam"], LENGTHS, w, h, valid=valid, frame_id=fid)
    keep = valid == 1
    for a, b in ((Rn, Rz), (Bn, Bz), (Cn, Cz)):
        assert np.isfinite(a[keep]).all() and a[keep].tobytes() == b[keep].tobytes() and np.isnan(a[bad]).all()
    assert Rn[keep].tobytes() == R[keep].tobytes()


def case_copies(be):
    """h = 0 returns the input bytes (whatever they are: a NaN too)."""
    x = make_inputs()
    x["rotmat"][5, 3, 2] = np.nan
    rc, R, B, C = run(be, x["rotmat"], x["betas"], x["cam"], LENGTHS, np.ones(1, np.float32), 0)
    assert rc == 0
    assert R.tobytes() == x["rotmat"].tobytes() and B.tobytes() == x["betas"].tobytes() and C.tobytes() == x["cam"].tobytes()


def case_nonfinite_taps(be):
    """A VALID frame whose matrix has no finite quaternion: left out of its neighbours' sums, itself copied."""
    x = make_inputs()
    off = offsets_of(LENGTHS)
    i = off[4] + 20
    x["rotmat"][i, 2] = np.nan
    w = gaussian(4)
    rc, R, B, C = run(be, x["rotmat"], x["betas"], x["cam"], LENGTHS, w, 4)
    ref = ref_smooth(x["rotmat"], x["betas"], x["cam"], LENGTHS, w, 4)
    assert rc == 0 and R[i, 2].tobytes() == x["rotmat"][i, 2].tobytes()
    R[i, 2] = ref[0][i, 2] = 0
    check((R, B, C), ref)


def case_determinism(be):
    x = make_inputs()
    w = gaussian(4)
    a = run(be, x["rotmat"], x["betas"], x["cam"], LENGTHS, w, 4)
    b = run(be, x["rotmat"], x["betas"], x["cam"], LENGTHS, w, 4)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(a[1:], b[1:]))


def case_position_independence(be):
    """The sequences in another order: every sequence's bytes are unchanged; one sequence's data changed: the others' bytes too."""
    x = make_inputs()
    w = gaussian(4)
    off = offsets_of(LENGTHS)
    base = run(be, x["rotmat"], x["betas"], x["cam"], LENGTHS, w, 4)[1:]
    perm = [4, 6, 0, 5, 3, 1, 2]
    idx = np.concatenate([np.arange(off[s], off[s + 1]) for s in perm]).astype(int)
    lens = [LENGTHS[s] for s in perm]
    got = run(be, x["rotmat"][idx], x["betas"][idx], x["cam"][idx], lens, w, 4)[1:]
    for a, b in zip(base, got):
        assert a[idx].tobytes() == b.tobytes()
    y = {k: v.copy() for k, v in x.items()}
    other = make_inputs(seed=99)
    for k in ("rotmat", "betas", "cam"):
        y[k][off[4]:off[5]] = other[k][off[4]:off[5]]
    got = run(be, y["rotmat"], y["betas"], y["cam"], LENGTHS, w, 4)[1:]
    rest = np.r_[0:off[4], off[5]:off[7]]
    for a, b in zip(base, got):
        assert a[rest].tobytes() == b[rest].tobytes() and a[off[4]:off[5]].tobytes() != b[off[4]:off[5]].tobytes()


def case_arguments(be):
    x = make_inputs((3, 5), 4, 2, 3, seed=5)
    w = gaussian(2)
    nan_w, neg_w, zero_c = w.copy(), w.copy(), w.copy()
    nan_w[0], neg_w[4], zero_c[2] = np.nan, -0.1, 0.0
    inf_w = w.copy()
    inf_w[1] = np.inf
    for kw in (dict(null=("rotmat",)), dict(null=("rotmat_out",)), dict(null=("off",)), dict(null=("weights",)), dict(null=("betas_out",)),
               dict(null=("cam_out",)), dict(alias="rotmat"), dict(alias="betas"), dict(alias="cam"), dict(h=-1), dict(h=33),
               dict(weights=nan_w), dict(weights=neg_w), dict(weights=zero_c), dict(weights=inf_w), dict(J=0), dict(n=-1), dict(n_seq=0),
               dict(nb=-1), dict(nc=-1)):
        kw = dict(kw)
        h = kw.pop("h", 2)
        ww = kw.pop("weights", w if h == 2 else np.ones(67, np.float32))
        rc, R, B, C = run(be, x["rotmat"], x["betas"], x["cam"], (3, 5), ww, h, **kw)
        assert rc == ERR_ARG, kw
        for name, o in (("rotmat", R), ("betas", B), ("cam", C)):
            if kw.get("alias") != name:
                assert (o == SENTINEL).all(), kw
    rc, R, B, C = run(be, x["rotmat"][:0], x["betas"][:0], x["cam"][:0], (0, 0), w, 2)                    # no frames: nothing to do
    assert rc == 0
    rc, R, B, C = run(be, x["rotmat"], None, None, (3, 5), w, 2, null=("betas_out", "cam_out"))          # no channels: no outputs needed
    assert rc == 0 and (R != SENTINEL).all()


# ------------------------------------------------------------------------------------------------------------------ the purpose
def accel_ratio(raw, smooth, clean, lengths):
    """mean |second difference of (X - clean)| over the triples inside sequences, raw over smoothed."""
    off = offsets_of(lengths)
    num = den = 0.0
    for a, b in zip(off[:-1], off[1:]):
        if b - a < 3:
            continue
        d2 = lambda X: (X[a:b - 2] - 2 * X[a + 1:b - 1] + X[a + 2:b])
        num += np.abs(d2(raw.astype(np.float64)) - d2(clean)).sum()
        den += np.abs(d2(smooth.astype(np.float64)) - d2(clean)).sum()
    return num / den


def case_purpose(be):
    """h = 4, sigma = 2: the second difference of the rotation matrices against the clean trajectory's falls at least 10 x with the
    restatement alone (measured 28 x), and the kernel's ratio lies within 1 % of the restatement's."""
    x = make_inputs()
    w = gaussian(4, 2.0)
    ref = ref_smooth(x["rotmat"], x["betas"], x["cam"], LENGTHS, w, 4)[0]
    r_ref = accel_ratio(x["rotmat"], ref, x["clean_rotmat"], LENGTHS)
    assert r_ref >= 10.0, r_ref
    rc, R, _, _ = run(be, x["rotmat"], x["betas"], x["cam"], LENGTHS, w, 4)
    r_k = accel_ratio(x["rotmat"], R, x["clean_rotmat"], LENGTHS)
    assert rc == 0 and abs(r_k / r_ref - 1) <= 0.01, (r_k, r_ref)


# ------------------------------------------------------------------------------------------------------------------ One-Euro
OE = dict(te=1 / 30.0, min_cutoff=1.0, beta=0.5, d_cutoff=1.0)
OE_R, OE_STEPS = 3, 12


def oe_stream():
    """R = 3 sequences x 12 steps from the recipe of make_inputs -> rotmat [steps][R][J][9], betas [steps][R][nb], cam [steps][R][nc]."""
    x = make_inputs((OE_STEPS,) * OE_R, seed=31)
    f = lambda a: np.ascontiguousarray(a.reshape(OE_R, OE_STEPS, *a.shape[1:]).swapaxes(0, 1))
    return f(x["rotmat"]), f(x["betas"]), f(x["cam"])


def oe_floats(be, Jn=J, nb=NB, nc=NC):
    n = be.lib.dyb_one_euro_state_floats(Jn, nb, nc)
    assert n == 1 + 2 * (4 * Jn + nb + nc)
    return n


def oe_step(be, state, rot, betas, cam, active=None, null=(), R=None, Jn=None, nb=None, nc=None, alias=None, outs=None, **par):
    """One dyb_one_euro_step on the backend buffer `state` -> (rc, rotmat_out, betas_out, cam_out) on the host; `outs`: prefilled
    output buffers to write into (default: SENTINEL)."""
    par = {**OE, **par}
    a = dict(state=state, rotmat=be.dev(rot), betas=be.dev(betas), cam=be.dev(cam), active=None if active is None else be.dev(active, np.uint8))
    o = outs or [be.dev(np.full(v.shape, SENTINEL, np.float32)) for v in (rot, betas, cam)]
    a.update(rotmat_out=o[0], betas_out=o[1], cam_out=o[2])
    p = {k: (None if k in null else be.ptr(v)) for k, v in a.items()}
    if alias:
        p[alias + "_out"] = p[alias]
    rc = be.lib.dyb_one_euro_step(p["state"], p["rotmat"], p["betas"], betas.shape[1] if nb is None else nb, p["cam"],
                                  cam.shape[1] if nc is None else nc, p["active"], par["te"], par["min_cutoff"], par["beta"], par["d_cutoff"],
                                  p["rotmat_out"], p["betas_out"], p["cam_out"], rot.shape[0] if R is None else R,
                                  rot.shape[1] if Jn is None else Jn, be.stream)
    return (rc, *(be.host(v) for v in o))


def oe_reference(dt, steps=OE_STEPS, **par):
    """The stream through the restatement: sequence 1 inactive at steps 4 - 5, sequence 2 reset before step 7 -> per step (outputs,
    active)."""
    rot, betas, cam = oe_stream()
    par = {**OE, **par}
    state = [dict(started=False, xh=None, dxh=None) for _ in range(OE_R)]
    out = []
    for t in range(steps):
        active = np.array([1, 0 if t in (4, 5) else 1, 1], np.uint8)
        if t == 7:
            state[2] = dict(started=False, xh=None, dxh=None)
        out.append((ref_one_euro_step(state, rot[t], betas[t], cam[t], active, dt=dt, **par), active))
    return out


def measure_oe_floor():
    a, b = oe_reference(np.float32), oe_reference(np.float64)
    worst = 0.0
    for (oa, act), (ob, _) in zip(a, b):
        on = act == 1
        worst = max(worst, *(float(np.abs(p[on].astype(np.float64) - q[on]).max()) for p, q in zip(oa, ob)))
    return worst


def case_oe_stream(be):
    rot, betas, cam = oe_stream()
    ref = oe_reference(np.float64)
    state = be.zeros((OE_R, oe_floats(be)))
    for t in range(OE_STEPS):
        (r_ref, active) = ref[t]
        if t == 7:
            s = be.host(state)
            s[2] = 0
            state = be.dev(s)
        before = be.host(state)
        rc, R, B, C = oe_step(be, state, rot[t], betas[t], cam[t], active)
        after = be.host(state)
        assert rc == 0
        on = active == 1
        check((R[on], B[on], C[on]), [v[on] for v in r_ref], OE_BOUND)
        check_orthonormal(R[on], OE_BOUND)
        first = t == 0
        for r in range(OE_R):
            if not active[r]:                                             # state and output bytes untouched
                assert after[r].tobytes() == before[r].tobytes()
                assert (R[r] == SENTINEL).all() and (B[r] == SENTINEL).all() and (C[r] == SENTINEL).all()
            elif first or (t == 7 and r == 2):                            # the first step and the step after a reset: the input bytes
                assert R[r].tobytes() == rot[t][r].tobytes() and B[r].tobytes() == betas[t][r].tobytes() and C[r].tobytes() == cam[t][r].tobytes()
                assert after[r, 0] == 1 and (after[r, 1 + 4 * J + NB + NC:] == 0).all()
            else:
                assert R[r].tobytes() != rot[t][r].tobytes() and after[r, 0] == 1
        q = after[on][:, 1:1 + 4 * J].reshape(-1, 4).astype(np.float64)
        assert np.abs((q * q).sum(-1) - 1).max() <= OE_BOUND           # stored normalised


def case_oe_closed_form(be):
    """beta = 0: the scalar channels are the exponential filter y_t = a x_t + (1 - a) y_(t-1), a = alpha(min_cutoff)."""
    rot, betas, cam = oe_stream()
    state = be.zeros((OE_R, oe_floats(be)))
    te, mc = OE["te"], 2.0
    a = 1.0 / (1.0 + (1.0 / (2 * np.pi * mc)) / te)
    yb, yc = betas[0].astype(np.float64), cam[0].astype(np.float64)
    for t in range(6):
        rc, R, B, C = oe_step(be, state, rot[t], betas[t], cam[t], None, beta=0.0, min_cutoff=mc)
        if t:
            yb, yc = a * betas[t] + (1 - a) * yb, a * cam[t] + (1 - a) * yc
        assert rc == 0 and np.abs(B - yb).max() <= OE_BOUND and np.abs(C - yc).max() <= OE_BOUND


def case_oe_arguments(be):
    rot, betas, cam = oe_stream()
    nfl = oe_floats(be)
    assert be.lib.dyb_one_euro_state_floats(0, 1, 1) == ERR_ARG and be.lib.dyb_one_euro_state_floats(1, -1, 0) == ERR_ARG
    assert be.lib.dyb_one_euro_state_floats(1, 0, 0) == 9
    for kw in (dict(null=("state",)), dict(null=("rotmat",)), dict(null=("rotmat_out",)), dict(null=("betas",)), dict(null=("betas_out",)),
               dict(null=("cam",)), dict(null=("cam_out",)), dict(alias="rotmat"), dict(alias="betas"), dict(alias="cam"), dict(te=0.0),
               dict(te=-1.0), dict(min_cutoff=0.0), dict(d_cutoff=0.0), dict(d_cutoff=-2.0), dict(beta=-1.0), dict(te=float("nan")),
               dict(Jn=0), dict(R=-1), dict(nb=-1), dict(nc=-1)):
        state = be.dev(np.full((OE_R, nfl), SENTINEL, np.float32))
        rc, R, B, C = oe_step(be, state, rot[0], betas[0], cam[0], None, **kw)
        assert rc == ERR_ARG, kw
        assert (be.host(state) == SENTINEL).all(), kw
        for name, o in (("rotmat", R), ("betas", B), ("cam", C)):
            if kw.get("alias") != name:
                assert (o == SENTINEL).all(), kw
