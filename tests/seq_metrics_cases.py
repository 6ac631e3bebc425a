"""Backend-agnostic checks of dyb_seq_metrics (csrc/seq_metrics.hip): each takes a backend of tests/backends.py, so the same cases run
on the kernel emulator and on the device.  The inputs are seeded and shared with tools/make_golden_seq_metrics.py, which stores the
REFERENCE's outputs on them (tests/golden/g14_seq_metrics.npz); the NumPy surface of dynaboa_amd/pose_utils.py is the second checker.

One ragged batch per joint count: sequence lengths 1, 2 (no triple), 3 (one triple), 0 (an empty row), 64 / 65 (the boundary of a
64-thread block), 130 (a boundary inside a block).  Neighbouring sequences are drawn from different distributions - an own offset of
the prediction of up to 0.8 m and an own noise level - so a triple that crossed a sequence boundary would carry the jump of the
offset: orders of magnitude above the sequence's own acceleration error.

Tolerances: the kernel works in double on fp32 inputs and rounds once to fp32, so columns 0 and 4 and the per-sequence means are
held to 1e-7 + 3 * 2^-24 |ref| (one rounding is 2^-24 |ref|; the means round a second time and read columns that were rounded
already).  PA-MPJPE keeps the bound of kernel_cases.case_pa_mpjpe, 2e-5 + 1e-4 max (Jacobi against LAPACK).  PCK and AUC are counts
over J (x the thresholds) and exact to 1e-6, because no joint distance lies within MARGIN of a threshold (asserted on these inputs);
flags and triple counts are exact."""
import numpy as np

from dynaboa_amd import pose_utils as PU

LENGTHS = (1, 2, 3, 0, 64, 65, 130)
JOINTS = (14, 17)
PCK_THR = 0.15
THRESHOLDS = np.linspace(0, 150, 31) / 1000
MARGIN = 1e-6
SENTINEL = 123.5
FF, SF = PU.FRAME_FLOATS, PU.SEQ_FLOATS
ERR_ARG = -1

OFFSET = (0.0, 0.4, 0.05, 0.0, 0.8, 0.02, 0.3)            # metres, |offset of the prediction| per sequence
NOISE = (0.004, 0.03, 0.01, 0.01, 0.002, 0.05, 0.02)      # metres, per-coordinate sigma of the prediction's error


def distances(pred, gt):
    return np.linalg.norm(pred.astype(np.float64) - gt.astype(np.float64), axis=-1)


def margin(pred, gt):
    """The smallest gap between a joint distance and a threshold (PCK's or any of the AUC's)."""
    thr = np.concatenate([[PCK_THR], THRESHOLDS])
    return float(np.abs(distances(pred, gt)[..., None] - thr).min())


def make_batch(J, seed=None):
    """-> (pred, gt) fp32 [sum(LENGTHS)][J][3]: a smooth ground-truth motion per sequence, the prediction = it + the sequence's offset
    + noise.  Joints that land within MARGIN of a threshold are pushed away (their error scaled by 1.0007, as often as needed)."""
    rng = np.random.default_rng(1400 + J if seed is None else seed)
    pred, gt = [], []
    for s, n in enumerate(LENGTHS):
        t = np.arange(n)[:, None, None] / 25.0
        base = rng.normal(0, 0.3, (1, J, 3))
        g = base + 0.2 * np.sin(2.0 * t + rng.uniform(0, 6, (1, J, 3))) + rng.normal(0, 0.002, (n, J, 3))
        d = rng.normal(0, 1, 3)
        p = g + OFFSET[s] * d / np.linalg.norm(d) + rng.normal(0, NOISE[s], (n, J, 3))
        pred.append(p); gt.append(g)
    pred, gt = np.concatenate(pred).astype(np.float32), np.concatenate(gt).astype(np.float32)
    thr = np.concatenate([[PCK_THR], THRESHOLDS])
    for _ in range(64):
        close = np.abs(distances(pred, gt)[..., None] - thr).min(-1) < 2 * MARGIN
        if not close.any():
            break
        pred[close] = (gt[close] + (pred[close] - gt[close]) * np.float32(1.0007)).astype(np.float32)
    assert margin(pred, gt) >= MARGIN
    return pred, gt


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)


def vis_mid():
    """`valid` with one invisible frame in the middle of the 65-frame sequence."""
    v = np.ones(sum(LENGTHS), np.uint8)
    v[offsets_of(LENGTHS)[5] + 32] = 0
    return v


def run(be, pred, gt, lengths, valid=None, frame_id=None, pck_thr=PCK_THR, thresholds=THRESHOLDS, J=None, n=None, n_seq=None,
        n_thr=None, null=()):
    """-> (rc, frame [n][FF], seq [n_seq + 1][SF]); the outputs start filled with SENTINEL.  `null`: argument names passed as NULL."""
    N = pred.shape[0]
    off = offsets_of(lengths)
    thr = np.asarray(thresholds, np.float32)
    frame = be.dev(np.full((max(N, 1), FF), SENTINEL, np.float32))
    seq = be.dev(np.full((len(lengths) + 1, SF), SENTINEL, np.float32))
    a = dict(pred=be.dev(pred), gt=be.dev(gt), off=be.dev(off, np.int32), valid=None if valid is None else be.dev(valid, np.uint8),
             fid=None if frame_id is None else be.dev(frame_id, np.int32), thr=be.dev(thr if thr.size else np.zeros(1, np.float32)),
             frame=frame, seq=seq)
    p = {k: (None if k in null else be.ptr(v)) for k, v in a.items()}
    rc = be.lib.dyb_seq_metrics(p["pred"], p["gt"], p["off"], len(lengths) if n_seq is None else n_seq, p["valid"], p["fid"],
                                float(pck_thr), p["thr"], int(thr.size) if n_thr is None else n_thr, p["frame"], p["seq"],
                                N if n is None else n, pred.shape[1] if J is None else J, be.stream)
    return rc, be.host(frame)[:N], be.host(seq)


def ref_frames(pred, gt, lengths, valid=None, frame_id=None, pck_thr=PCK_THR, thresholds=THRESHOLDS):
    """The NumPy surface of pose_utils on float64 copies -> frame [n][FF] (float64)."""
    p, g = pred.astype(np.float64), gt.astype(np.float64)
    n = p.shape[0]
    out = np.zeros((n, FF))
    out[:, 0] = distances(pred, gt).mean(-1)
    if n:
        out[:, 1] = PU.reconstruction_error(p, g, reduction=None)
        out[:, 2] = PU.compute_pck(p, g, pck_thr)
        out[:, 3] = np.mean([PU.compute_pck(p, g, t) for t in thresholds], 0) if len(thresholds) else 0.0
    off = offsets_of(lengths)
    for s in range(len(lengths)):
        a, b = off[s], off[s + 1]
        if b - a < 3:
            continue
        acc = PU.compute_error_accel(g[a:b], p[a:b])                          # one value per triple, centre a + 1 + k
        ok = np.ones(b - a - 2, bool)
        if valid is not None:
            v = valid[a:b].astype(bool)
            ok &= v[:-2] & v[1:-1] & v[2:]
            assert np.array_equal(acc[ok], PU.compute_error_accel(g[a:b], p[a:b], v))     # the reference's own masking agrees
        if frame_id is not None:
            f = np.asarray(frame_id[a:b], np.int64)
            ok &= (f[1:-1] == f[:-2] + 1) & (f[2:] == f[1:-1] + 1)
        out[a + 1:b - 1, 4] = np.where(ok, acc, 0.0)
        out[a + 1:b - 1, 5] = ok
    return out


def ref_seq(frame, lengths):
    """Per-sequence rows from per-frame columns, in double -> [len(lengths) + 1][SF]."""
    off = offsets_of(lengths)
    rows = []
    for a, b in list(zip(off[:-1], off[1:])) + [(0, off[-1])]:
        f = frame[a:b].astype(np.float64)
        c = f[:, 5] > 0.5
        rows.append([b - a, *(f[:, k].mean() if b > a else 0.0 for k in range(4)), f[c, 4].mean() if c.any() else 0.0, c.sum()])
    return np.asarray(rows, np.float64)


def tight(got, ref):
    return np.abs(got - ref) <= 1e-7 + 3 * 2.0 ** -24 * np.abs(ref)


def check_frames(got, ref):
    assert tight(got[:, 0], ref[:, 0]).all(), np.abs(got[:, 0] - ref[:, 0]).max()
    if len(ref):
        assert np.abs(got[:, 1] - ref[:, 1]).max() <= 2e-5 + 1e-4 * ref[:, 1].max(), np.abs(got[:, 1] - ref[:, 1]).max()
    assert (np.abs(got[:, 2:4] - ref[:, 2:4]) <= 1e-6).all(), np.abs(got[:, 2:4] - ref[:, 2:4]).max()
    assert tight(got[:, 4], ref[:, 4]).all(), np.abs(got[:, 4] - ref[:, 4]).max()
    assert np.array_equal(got[:, 5], ref[:, 5])
    assert (got[got[:, 5] == 0, 4] == 0).all() and np.isfinite(got).all()


def check_seq(got, frame_got, lengths, ref_frame=None):
    """The rows against the means, in double, of the kernel's OWN per-frame columns (what the reduction is given) and, with
    `ref_frame`, against the means of the NumPy surface's columns."""
    ref = ref_seq(frame_got, lengths)
    assert np.array_equal(got[:, 0], ref[:, 0]) and np.array_equal(got[:, 6], ref[:, 6])
    assert tight(got[:, 1:6], ref[:, 1:6]).all(), np.abs(got[:, 1:6] - ref[:, 1:6]).max()
    for s, n in enumerate(lengths):
        if n == 0:
            assert (got[s] == 0).all()
    if ref_frame is not None:
        ref = ref_seq(ref_frame, lengths)
        assert np.array_equal(got[:, 0], ref[:, 0]) and np.array_equal(got[:, 6], ref[:, 6])
        assert tight(got[:, [1, 5]], ref[:, [1, 5]]).all(), np.abs(got[:, [1, 5]] - ref[:, [1, 5]]).max()
        assert np.abs(got[:, 2] - ref[:, 2]).max() <= 2e-5 + 1e-4 * ref_frame[:, 1].max()
        assert (np.abs(got[:, 3:5] - ref[:, 3:5]) <= 1e-6).all()


def case_batch(be, golden, J):
    """The ragged batch against the golden (reference output) and against the NumPy surface."""
    pred, gt = make_batch(J)
    assert margin(pred, gt) >= MARGIN
    g = golden("g14_seq_metrics.npz")
    assert np.array_equal(g[f"pred{J}"], pred) and np.array_equal(g[f"gt{J}"], gt)      # the golden was made from these inputs
    rc, frame, seq = run(be, pred, gt, LENGTHS)
    assert rc == 0
    ref = ref_frames(pred, gt, LENGTHS)
    check_frames(frame, ref)
    check_seq(seq, frame, LENGTHS, ref)
    # the reference itself: reconstruction_error(needpck, needauc) of every single sample, compute_error_accel of every sequence
    assert np.abs(frame[:, 1] - g[f"re{J}"]).max() <= 2e-5 + 1e-4 * g[f"re{J}"].max()
    assert np.abs(frame[:, 2] - g[f"pck{J}"]).max() <= 1e-6 and np.abs(frame[:, 3] - g[f"auc{J}"]).max() <= 1e-6
    off = offsets_of(LENGTHS)
    triples = 0
    for s, n in enumerate(LENGTHS):
        if n >= 3:
            a = g[f"accel{J}_s{s}"]
            assert tight(frame[off[s] + 1:off[s + 1] - 1, 4], a).all() and (frame[off[s] + 1:off[s + 1] - 1, 5] == 1).all()
            assert tight(seq[s, 5], a.mean()) and seq[s, 6] == n - 2
            triples += n - 2
        for i in {off[s], off[s + 1] - 1} if n else ():
            assert frame[i, 4] == 0 and frame[i, 5] == 0                                # no triple is centred on a sequence's end
    assert seq[-1, 6] == triples == 1 + 62 + 63 + 128 and seq[-1, 0] == sum(LENGTHS)


def case_masks(be, golden, J=14):
    pred, gt = make_batch(J)
    g = golden("g14_seq_metrics.npz")
    off = offsets_of(LENGTHS)
    _, base, base_seq = run(be, pred, gt, LENGTHS)
    # one invisible frame in the middle of the 65-frame sequence: exactly three triples go, and the rest is compute_error_accel(vis)
    v = vis_mid()
    assert np.array_equal(g["vis"], v)
    rc, frame, seq = run(be, pred, gt, LENGTHS, valid=v)
    assert rc == 0
    ref = ref_frames(pred, gt, LENGTHS, valid=v)
    check_frames(frame, ref)
    check_seq(seq, frame, LENGTHS, ref)
    gone = np.flatnonzero(base[:, 5] != frame[:, 5])
    assert gone.tolist() == [off[5] + 31, off[5] + 32, off[5] + 33]
    kept = frame[off[5]:off[6], 5] == 1
    assert tight(frame[off[5]:off[6], 4][kept], g[f"accel_vis{J}_s5"]).all() and kept.sum() == 60 == seq[5, 6]
    assert np.array_equal(frame[:, :4], base[:, :4])                                   # the mask touches the triples only
    # invisible first and last frames each remove one triple
    v = np.ones(sum(LENGTHS), np.uint8)
    v[off[6]] = v[off[7] - 1] = 0
    rc, frame, seq = run(be, pred, gt, LENGTHS, valid=v)
    assert np.flatnonzero(base[:, 5] != frame[:, 5]).tolist() == [off[6] + 1, off[7] - 2] and seq[6, 6] == 126
    check_frames(frame, ref_frames(pred, gt, LENGTHS, valid=v))
    # frame ids with one gap (between local frames 9 and 10 of the 64-frame sequence): the two triples that straddle it go
    fid = np.concatenate([np.arange(n) + 7 * s for s, n in enumerate(LENGTHS)]).astype(np.int32)
    rc, frame, seq = run(be, pred, gt, LENGTHS, frame_id=fid)
    assert np.array_equal(frame, base) and np.array_equal(seq, base_seq)               # consecutive ids change nothing
    fid[off[4] + 10:off[5]] += 3
    rc, frame, seq = run(be, pred, gt, LENGTHS, frame_id=fid)
    assert np.flatnonzero(base[:, 5] != frame[:, 5]).tolist() == [off[4] + 9, off[4] + 10] and seq[4, 6] == 60
    check_frames(frame, ref_frames(pred, gt, LENGTHS, frame_id=fid))
    check_seq(seq, frame, LENGTHS)


def case_determinism(be, J=17):
    pred, gt = make_batch(J)
    v = vis_mid()
    _, f1, s1 = run(be, pred, gt, LENGTHS, valid=v)
    _, f2, s2 = run(be, pred, gt, LENGTHS, valid=v)
    assert f1.tobytes() == f2.tobytes() and s1.tobytes() == s2.tobytes()
    off = offsets_of(LENGTHS)
    for s, n in enumerate(LENGTHS):                                                     # one call per sequence: the same rows
        a, b = off[s], off[s + 1]
        rc, f, q = run(be, pred[a:b], gt[a:b], [n], valid=v[a:b])
        assert rc == 0 and f.tobytes() == f1[a:b].tobytes()
        assert q[0].tobytes() == s1[s].tobytes() and q[1].tobytes() == s1[s].tobytes(), s


def case_arguments(be, J=14):
    pred, gt = make_batch(J)
    for kw in (dict(null=("pred",)), dict(null=("gt",)), dict(null=("off",)), dict(null=("frame",)), dict(null=("seq",)),
               dict(null=("thr",)), dict(J=2), dict(n=-1), dict(n_seq=0), dict(n_thr=-1), dict(n_thr=65)):
        rc, frame, seq = run(be, pred, gt, LENGTHS, **kw)
        assert rc == ERR_ARG, kw
        assert (frame == SENTINEL).all() and (seq == SENTINEL).all(), kw
    rc, frame, seq = run(be, pred, gt, LENGTHS, thresholds=[])                          # no thresholds: AUC 0, nothing else changes
    _, base, _ = run(be, pred, gt, LENGTHS)
    assert rc == 0 and (frame[:, 3] == 0).all() and (seq[:, 4] == 0).all() and np.array_equal(frame[:, [0, 1, 2, 4, 5]], base[:, [0, 1, 2, 4, 5]])
    rc, frame, seq = run(be, pred, gt, LENGTHS, pck_thr=0.0, thresholds=[0.0])          # strict <: nothing is closer than 0
    assert rc == 0 and (frame[:, 2] == 0).all() and (frame[:, 3] == 0).all()
    rc, frame, seq = run(be, pred[:0], gt[:0], [0, 0])                                  # no frames at all: rows of zeros
    assert rc == 0 and (seq == 0).all()
