"""Backend-agnostic checks of dyb_track_videos (csrc/track.hip): each takes a backend of tests/backends.py, so the same cases run on the
kernel emulator and on the device.  The reference has no tracker; the oracle is `ref_track` below, a restatement of the rule of
include/dynaboa_hip.h in NumPy, evaluated in float64 (and in float32, for the tolerance).

The scene (seeded, `make_scene`): 60 frames, 6 people, K = 17, bodies of 80 x 200 pixels from one template per person plus 0.5 pixels
of noise per joint and frame.  People 1 and 2 share a template and pass each other 18 pixels apart at 1.5 pixels per frame each, so
that for several frames a track has two candidates above s_min; person 3 is missing for 3 frames (frames 20 - 22: the gap of 4 frame
ids is within max_age = 5 and the id stays); person 4 is missing for 20 frames (10 - 29) and comes back under a new id; person 5
enters at frame 15.  Two joints of every detection are hidden (confidence 0.1), the order of a frame's detections is shuffled, and
frame 40 holds one more detection with two visible joints.  Expected: 7 tracks, each holding one person.

Conditions on the scene, asserted by test_track_kernels.py::test_scene_conditions on the float64 restatement: within every frame any
two candidate similarities (>= s_min) differ by at least MARGIN, and no similarity lies within MARGIN of s_min - so no rounding can
decide an assignment and ids are compared for EQUALITY; at least 3 frames are ambiguous (a track with two candidates); both gap
behaviours occur.  The seed was searched for the gap (seeds 0 .. 39: the smallest gap ranged from 2.6e-7 to 7.7e-5, every seed gave
7 tracks of one person each, 5 - 6 ambiguous frames and equal ids from the float32 and the float64 evaluation).
  seed 19: smallest gap 5.62e-5, nearest similarity to s_min 1.5e-3, 6 ambiguous frames   (MARGIN 2e-5)

Tolerance of sim_out.  The restatement is evaluated in float32 and in float64 on the scene; the bound is 8 x the largest difference -
room for FMA contraction and a device expf that is not correctly rounded.  (In float32 the restatement takes exp in float64 and
rounds once: NumPy's float32 exp differs in the last bit between CPUs, and the floor must not.)
  measured floor 1.57e-7 -> FLOOR 1.6e-7, BOUND 1.28e-6
test_track_kernels.py::test_scene_conditions asserts that the measured floor lies in (FLOOR / 2, FLOOR] and that FLOOR <= MARGIN / 100."""
import numpy as np

MAX_PEOPLE, MAX_KP, VIDEO_INTS = 64, 32, 4
SENTINEL_I, SENTINEL_F = -77, 123.5
GUARD = 8                                      # sentinel elements behind the n a call is given
ERR_ARG = -1
RULE = dict(c_min=0.3, kappa=0.1, s_min=0.3, max_age=5, min_common=3)
MARGIN = 2e-5
FLOOR = 1.6e-7
BOUND = 8 * FLOOR
SCENE_SEED = 19
SCENE_K, SCENE_FRAMES = 17, 60


# ------------------------------------------------------------------------------------------------------------------ packing
def pack(videos, K=None):
    """videos: a list of videos, each a list of per-frame (n_f, K, 3) arrays -> (kp [n][K][3] fp32, det_offsets [F + 1],
    frame_offsets [V + 1])."""
    frames = [np.asarray(f, np.float32) for v in videos for f in v]
    if K is None:
        K = next((f.shape[1] for f in frames if f.ndim == 3), 1)
    frames = [f.reshape(-1, K, 3) for f in frames]
    kp = np.concatenate(frames) if frames else np.zeros((0, K, 3), np.float32)
    det = np.concatenate([[0], np.cumsum([f.shape[0] for f in frames])]).astype(np.int32)
    fr = np.concatenate([[0], np.cumsum([len(v) for v in videos])]).astype(np.int32)
    return np.ascontiguousarray(kp, np.float32), det, fr


# ------------------------------------------------------------------------------------------------------------------ the restatement
def ref_track(kp, det_off, frame_off, frame_id=None, *, c_min, kappa, s_min, max_age, min_common, dt=np.float64, diag=None):
    """The rule of dyb_track_videos, arithmetic in `dt` on the float32 inputs (the parameters are the C floats) -> (track [n] int32,
    sim [n] dt, video [V][4] int32).  diag (a list): one dict per frame with the similarity matrix `S` [live tracks][detections]."""
    kp = np.asarray(kp, np.float32)
    n, K = kp.shape[0], kp.shape[1]
    cm, ka, sm = np.float32(c_min), dt(np.float32(kappa)), dt(np.float32(s_min))
    track, sim = -np.ones(n, np.int32), -np.ones(n, dt)
    video = np.zeros((len(frame_off) - 1, VIDEO_INTS), np.int32)
    for v in range(len(frame_off) - 1):
        tracks, next_id = [], 0                                        # in order of creation = ascending id
        for f in range(frame_off[v], frame_off[v + 1]):
            fid = int(frame_id[f]) if frame_id is not None else f - int(frame_off[v])
            tracks = [t for t in tracks if fid - t["last"] <= max_age]
            o0, o1 = int(det_off[f]), int(det_off[f + 1])
            m = min(o1 - o0, MAX_PEOPLE)
            video[v, 2] += (o1 - o0) - m
            dets = []
            for d in range(m):
                p = kp[o0 + d]
                mask = p[:, 2] > cm
                xy = p[:, :2].astype(dt)
                area = dt(0)
                if mask.any():
                    vis = xy[mask]
                    area = dt((vis[:, 0].max() - vis[:, 0].min()) * (vis[:, 1].max() - vis[:, 1].min()))
                dets.append(dict(xy=xy, mask=mask, area=area, ok=int(mask.sum()) >= min_common))
            S = np.zeros((len(tracks), m), dt)
            if tracks and m:
                txy, dxy = np.stack([t["xy"] for t in tracks]), np.stack([d["xy"] for d in dets])
                common = np.stack([t["mask"] for t in tracks])[:, None, :] & np.stack([d["mask"] & d["ok"] for d in dets])[None, :, :]
                nc = common.sum(-1)
                A = np.maximum((np.array([t["area"] for t in tracks], dt)[:, None] + np.array([d["area"] for d in dets], dt)[None, :]) * dt(0.5),
                               dt(1)).astype(dt)
                den = (dt(2) * ka * ka * A).astype(dt)
                acc = np.zeros((len(tracks), m), dt)
                for k in range(K):                                      # ascending k: the kernel's order of summation
                    dx, dy = txy[:, None, k, 0] - dxy[None, :, k, 0], txy[:, None, k, 1] - dxy[None, :, k, 1]
                    # exp in float64, rounded once to dt: in float32 the correctly rounded expf, the same on every host (NumPy's own
                    # float32 exp is a SIMD routine whose last bit depends on the CPU it runs on - the floor would move with it)
                    e = np.exp((-(dx * dx + dy * dy) / den).astype(dt).astype(np.float64)).astype(dt)
                    acc = np.where(common[:, :, k], acc + e, acc).astype(dt)
                S = np.where(nc >= min_common, acc / np.maximum(nc, 1).astype(dt), dt(0)).astype(dt)
            if diag is not None:
                diag.append(dict(video=v, frame=f, S=S.copy(), ids=[t["id"] for t in tracks]))
            t_free, d_free = np.ones(len(tracks), bool), np.array([d["ok"] for d in dets], bool)
            match = {}
            while True:
                cand = (S >= sm) & t_free[:, None] & d_free[None, :] if S.size else np.zeros((0, 0), bool)
                if not cand.any():
                    break
                best = S[cand].max()
                ti, di = [(a, b) for a, b in zip(*np.nonzero(cand & (S == best)))][0]      # row-major: lower id, then lower index
                match[int(di)] = int(ti)
                t_free[ti], d_free[di] = False, False
            for d in range(m):
                det = dets[d]
                if not det["ok"]:
                    video[v, 1] += 1
                    continue
                if d in match:
                    t = tracks[match[d]]
                    track[o0 + d], sim[o0 + d] = t["id"], S[match[d], d]
                elif len(tracks) < MAX_PEOPLE:
                    t = dict(id=next_id)
                    tracks.append(t)
                    track[o0 + d], sim[o0 + d] = next_id, dt(0)
                    next_id += 1
                    video[v, 0] += 1
                else:
                    video[v, 2] += 1
                    continue
                t.update(xy=det["xy"], mask=det["mask"], area=det["area"], last=fid)
    return track, sim, video


# ------------------------------------------------------------------------------------------------------------------ the scene
def body(rng, K, width=80.0, height=200.0):
    """A template: K joint offsets inside a width x height box whose corners are joints 0 and 1."""
    t = np.stack([rng.uniform(-width / 2, width / 2, K), rng.uniform(-height / 2, height / 2, K)], -1)
    if K >= 2:
        t[0], t[1] = (-width / 2, -height / 2), (width / 2, height / 2)
    return t


def make_scene(seed=SCENE_SEED, K=SCENE_K, frames=SCENE_FRAMES):
    """-> (video: a list of `frames` (n_f, K, 3) float32 arrays, person: per frame the person of every detection, -1 for the
    untrackable one)."""
    rng = np.random.default_rng(seed)
    tpl = [body(rng, K) for _ in range(6)]
    tpl[2] = tpl[1] + rng.normal(0, 0.5, (K, 2))                              # near-identical bodies
    path = [lambda f: (100 + 3.0 * f, 150.0), lambda f: (400 + 1.5 * f, 500.0), lambda f: (490 - 1.5 * f, 518.0),
            lambda f: (800 + 1.0 * f, 150.0), lambda f: (850 - 0.5 * f, 560.0), lambda f: (1150.0, 330 + 2.0 * f)]
    present = [lambda f: True, lambda f: True, lambda f: True, lambda f: not 20 <= f <= 22, lambda f: not 10 <= f <= 29, lambda f: f >= 15]
    video, person = [], []
    for f in range(frames):
        dets, who = [], []
        for p in range(6):
            if not present[p](f):
                continue
            xy = tpl[p] + np.array(path[p](f)) + rng.normal(0, 0.5, (K, 2))
            conf = rng.uniform(0.5, 0.95, K)
            conf[rng.choice(np.arange(2, K), 2, replace=False)] = 0.1       # two hidden joints (not the box corners)
            dets.append(np.concatenate([xy, conf[:, None]], -1))
            who.append(p)
        if f == 40:
            xy = body(rng, K) + np.array([1400.0, 700.0])
            conf = np.full(K, 0.05)
            conf[[3, 9]] = 0.9
            dets.append(np.concatenate([xy, conf[:, None]], -1))
            who.append(-1)
        order = rng.permutation(len(dets))
        video.append(np.stack([dets[i] for i in order]).astype(np.float32))
        person.append([who[i] for i in order])
    return video, person


def pad_joints(video, K):
    """The video with joints of confidence 0 appended up to K."""
    out = []
    for fr in video:
        p = np.zeros((fr.shape[0], K, 3), np.float32)
        p[:, :fr.shape[1]] = fr
        out.append(p)
    return out


def scene_conditions(seed=SCENE_SEED):
    """-> dict: smallest gap between two candidate similarities of one frame, smallest distance of a similarity from s_min, ambiguous
    frames (a track with two candidates), tracks, the fp32 / fp64 floor, whether every track holds one person, the ids of persons 3
    and 4 before and after their gaps."""
    video, person = make_scene(seed)
    kp, det, fr = pack([video])
    diag = []
    tr64, s64, vid = ref_track(kp, det, fr, dt=np.float64, diag=diag, **RULE)
    tr32, s32, _ = ref_track(kp, det, fr, dt=np.float32, **RULE)
    s_min = float(np.float32(RULE["s_min"]))
    gap, edge, ambiguous = np.inf, np.inf, 0
    for fd in diag:
        S = fd["S"]
        if not S.size:
            continue
        edge = min(edge, float(np.abs(S - s_min).min()))
        c = np.sort(S[S >= s_min])
        if c.size > 1:
            gap = min(gap, float(np.diff(c).min()))
        ambiguous += int(((S >= s_min).sum(1) > 1).any())
    who = np.concatenate([np.array(p) for p in person])
    pure = all(len(set(who[tr64 == t])) == 1 for t in set(tr64[tr64 >= 0]))
    at = lambda f, p: int(tr64[det[f] + person[f].index(p)])
    return dict(gap=gap, edge=edge, ambiguous=ambiguous, tracks=int(vid[0, 0]), untrackable=int(vid[0, 1]), pure=pure,
                floor=float(np.abs(s32.astype(np.float64) - s64).max()), ids_equal=bool(np.array_equal(tr32, tr64)),
                short_gap=(at(19, 3), at(23, 3)), long_gap=(at(9, 4), at(30, 4)), enters=at(15, 5))


# ------------------------------------------------------------------------------------------------------------------ the driver
def run(be, kp, det_off, frame_off, frame_id=None, null=(), n=None, F=None, V=None, K=None, want_sim=True, **rule):
    """-> (rc, track [n + GUARD], sim [n + GUARD] or None, video [V][4]); the outputs start filled with sentinels.  `null`: argument
    names passed as NULL."""
    par = {**RULE, **rule}
    kp = np.asarray(kp, np.float32)
    N, Kn = kp.shape[0], kp.shape[1]
    nv = len(frame_off) - 1
    a = dict(kp=be.dev(kp if N else np.zeros((1, Kn, 3))), det=be.dev(det_off, np.int32), fr=be.dev(frame_off, np.int32),
             fid=None if frame_id is None else be.dev(np.asarray(frame_id) if len(frame_id) else np.zeros(1), np.int32),
             track=be.dev(np.full(N + GUARD, SENTINEL_I), np.int32), sim=be.dev(np.full(N + GUARD, SENTINEL_F)) if want_sim else None,
             video=be.dev(np.full((max(nv, 1), VIDEO_INTS), SENTINEL_I), np.int32))
    p = {k: (None if k in null else be.ptr(v)) for k, v in a.items()}
    rc = be.lib.dyb_track_videos(p["kp"], p["det"], p["fr"], p["fid"], Kn if K is None else K, par["c_min"], par["kappa"], par["s_min"],
                                 int(par["max_age"]), int(par["min_common"]), p["track"], p["sim"], p["video"], N if n is None else n,
                                 len(det_off) - 1 if F is None else F, nv if V is None else V, be.stream)
    return rc, be.host(a["track"]), None if a["sim"] is None else be.host(a["sim"]), be.host(a["video"])


def check(be, videos, frame_ids=None, exact_sim=False, **rule):
    """Run `videos` and compare with the float64 restatement: ids and counts equal, sim within BOUND, the guard untouched.
    -> (track, sim, video) of the n detections."""
    kp, det, fr = pack(videos)
    fid = None if frame_ids is None else np.concatenate([np.asarray(x, np.int32) for x in frame_ids] + [np.zeros(0, np.int32)])
    rc, tr, sim, vid = run(be, kp, det, fr, fid, **rule)
    assert rc == 0
    n = kp.shape[0]
    rt, rs, rv = ref_track(kp, det, fr, fid, **{**RULE, **rule})
    assert (tr[n:] == SENTINEL_I).all() and (sim[n:] == SENTINEL_F).all()
    assert np.array_equal(tr[:n], rt), (tr[:n], rt)
    assert np.array_equal(vid, rv), (vid, rv)
    err = float(np.abs(sim[:n].astype(np.float64) - rs).max()) if n else 0.0
    assert np.isfinite(sim[:n]).all() and err <= BOUND, err
    return tr[:n], sim[:n], vid


def person(cx, cy, K=5, conf=0.9, w=40.0, h=100.0):
    """A detection with integer-valued coordinates: K joints on the diagonal of a w x h box centred on (cx, cy)."""
    t = np.linspace(-0.5, 0.5, K) if K > 1 else np.zeros(1)
    return np.stack([np.round(cx + w * t), np.round(cy + h * t), np.full(K, conf)], -1).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ the cases
def case_scene(be):
    """The scene alone, then as video 1 of a batch of 3 (video 0 has no frame, video 2 is the scene padded to K = 25 with joints of
    confidence 0): ids equal to the restatement, 7 tracks of one person each, the scene's output bytes the same in both positions
    and with the padding."""
    video, who = make_scene()
    tr, sim, vid = check(be, [video])
    who = np.concatenate([np.array(p) for p in who])
    assert vid.tolist() == [[7, 1, 0, 0]] and all(len(set(who[tr == t])) == 1 for t in range(7)) and (tr[who == -1] == -1).all()
    wide = pad_joints(video, 25)
    n = tr.shape[0]
    kp, det, fr = pack([[], wide, wide])
    rc, tr3, sim3, vid3 = run(be, kp, det, fr)
    assert rc == 0 and vid3.tolist() == [[0, 0, 0, 0], [7, 1, 0, 0], [7, 1, 0, 0]]
    for lo in (0, n):
        assert tr3[lo:lo + n].tobytes() == tr.tobytes() and sim3[lo:lo + n].tobytes() == sim.tobytes()
    assert (tr3[2 * n:] == SENTINEL_I).all() and kp.shape[1] == 25


def case_frame_ids(be):
    """A person seen at positions 0 and 4 of a video: consecutive ids keep the track at max_age = 5 (gap 4), every second number
    retires it (gap 8); max_age = 1 continues only adjacent frame ids, and max_age = 0 - the rule retires at frame_id - last >
    max_age - continues none."""
    a, b = person(200, 300), person(900, 300)
    video = [np.stack([a, b]), b[None], b[None], b[None], np.stack([a, b])]
    tr, _, vid = check(be, [video])
    assert tr.tolist() == [0, 1, 1, 1, 1, 0, 1] and vid[0, 0] == 2
    tr, _, vid = check(be, [video], frame_ids=[[0, 2, 4, 6, 8]], max_age=8)
    assert tr.tolist() == [0, 1, 1, 1, 1, 0, 1]
    tr, _, vid = check(be, [video], frame_ids=[[0, 2, 4, 6, 8]])
    assert tr.tolist() == [0, 1, 1, 1, 1, 2, 1] and vid[0, 0] == 3
    tr, _, _ = check(be, [[a[None]] * 4], frame_ids=[[0, 1, 3, 4]], max_age=1)        # frame_id - last > max_age: 1 keeps, 2 retires
    assert tr.tolist() == [0, 0, 1, 1]
    tr, _, _ = check(be, [[a[None]] * 4], frame_ids=[[0, 1, 3, 4]], max_age=0)        # the same inequality: even 1 retires
    assert tr.tolist() == [0, 1, 2, 3]
    tr, _, _ = check(be, [[a[None]] * 3, [a[None]] * 3], frame_ids=[[7, 8, 9], [5, 10, 11]], max_age=4)      # ids are per video
    assert tr.tolist() == [0, 0, 0, 0, 1, 1]


def case_ties(be):
    """Two bit-identical detections in each of three frames: ids (0, 1) every time - the older track takes the lower index.  Two
    live tracks equally similar to one detection (5 pixels to either side, integer coordinates: the same bits): the lower id wins."""
    a = person(300, 300)
    tr, sim, _ = check(be, [[np.stack([a, a])] * 3])
    assert tr.tolist() == [0, 1, 0, 1, 0, 1] and sim.tolist() == [0, 0, 1, 1, 1, 1]
    for first, second in ((295, 305), (305, 295)):
        video = [np.stack([person(first, 300), person(second, 300)]), person(300, 300)[None], np.stack([person(first, 300), person(second, 300)])]
        kp, det, fr = pack([video])
        diag = []
        ref_track(kp, det, fr, diag=diag, **RULE)
        assert diag[1]["S"][0, 0] == diag[1]["S"][1, 0] > 0.7                  # equal bits in the restatement too
        tr, sim, _ = check(be, [video])
        assert tr[:3].tolist() == [0, 1, 0]
        # frame 2: track 0 now stands in the middle, 5 pixels from both detections: it takes the lower index, track 1 the other
        assert tr[3:].tolist() == [0, 1]


def grid(count, K=5, shift=0.0):
    return np.stack([person(500 + 1000 * (i % 8) + shift, 500 + 1000 * (i // 8), K) for i in range(count)])


def case_limits(be):
    """Exactly 64 detections: ids 0 .. 63; 65: the last gets -1 and is counted; 64 live tracks: a newcomer gets -1 until a track
    retires, then the next id; a frame without detections; K = 1 with min_common = 1; K = 32."""
    tr, sim, vid = check(be, [[grid(64), grid(64, shift=3.0)]])
    assert tr.tolist() == list(range(64)) * 2 and vid.tolist() == [[64, 0, 0, 0]] and (sim[64:] > 0.85).all()
    tr, sim, vid = check(be, [[grid(65)]])
    assert tr.tolist() == list(range(64)) + [-1] and sim[64] == -1 and vid.tolist() == [[64, 0, 1, 0]]
    new = person(300, 9500)[None]
    later = np.concatenate([grid(64)[1:], new])                                 # person 0 has left; 63 tracks matched, 64 still live
    tr, sim, vid = check(be, [[grid(64), later, later, later]], max_age=2)
    assert tr[64:].tolist() == (list(range(1, 64)) + [-1]) * 2 + list(range(1, 64)) + [64]
    assert sim[127] == -1 and sim[255] == 0 and vid.tolist() == [[65, 0, 2, 0]]
    a = person(200, 300)
    tr, _, vid = check(be, [[a[None], np.zeros((0, 5, 3)), a[None]], [np.zeros((0, 5, 3))], [np.zeros((0, 5, 3))] * 3])
    assert tr.tolist() == [0, 0] and vid.tolist() == [[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    p, q = person(100, 100, K=1), person(103, 100, K=1)
    tr, sim, _ = check(be, [[np.stack([p, person(900, 100, K=1)]), np.stack([person(903, 100, K=1), q])]], min_common=1, kappa=10.0)
    assert tr.tolist() == [0, 1, 1, 0] and abs(sim[3] - np.exp(-9 / 200.0)) <= BOUND           # area 0 -> A = 1
    tr, _, _ = check(be, [[q[None], q[None]]])                                  # one joint is fewer than min_common = 3
    assert tr.tolist() == [-1, -1]
    rng = np.random.default_rng(3)
    tpl = [body(rng, 32) + c for c in ((200, 300), (600, 300), (1000, 300))]
    wide = [np.stack([np.concatenate([t + 2.0 * f, rng.uniform(0.2, 0.9, (32, 1))], -1) for t in tpl]) for f in range(4)]
    tr, _, vid = check(be, [wide])
    assert tr.tolist() == [0, 1, 2] * 4 and vid.tolist() == [[3, 0, 0, 0]]


def case_thresholds(be):
    """c_min is strict: a joint at exactly c_min is not visible.  A detection below min_common gets -1, is counted and leaves the
    tracks untouched."""
    c = np.float32(RULE["c_min"])
    a = person(200, 300, K=4)
    edge = a.copy()
    edge[:2, 2] = c                                                              # two of four joints at exactly c_min: two visible
    above = a.copy()
    above[:2, 2] = np.nextafter(c, np.float32(1))
    moved = person(206, 300, K=4)
    ghost = person(203, 300, K=4)
    ghost[:, 2] = c
    tr, sim, vid = check(be, [[a[None], edge[None], np.stack([ghost, moved])]])
    assert tr.tolist() == [0, -1, -1, 0] and sim[1] == -1 and vid.tolist() == [[1, 2, 0, 0]]
    # the track still stands where frame 0 left it: s is that of a 6-pixel step (3 pixels had the ghost moved it)
    _, s_ref, _ = ref_track(*pack([[a[None], moved[None]]]), **RULE)
    assert abs(sim[3] - s_ref[1]) <= BOUND
    tr, _, vid = check(be, [[a[None], above[None]]])
    assert tr.tolist() == [0, 0] and vid.tolist() == [[1, 0, 0, 0]]
    tr, _, _ = check(be, [[a[None], a[None]]], min_common=5)
    assert tr.tolist() == [-1, -1]
    tr, _, _ = check(be, [[a[None], person(200 + 150, 300, K=4)[None]]])        # far below s_min: a new track
    assert tr.tolist() == [0, 1]


def case_determinism(be):
    """Two calls return equal bytes in all three outputs; sentinel-filled outputs are overwritten for every detection and nothing is
    written past n; sim_out may be NULL."""
    video, _ = make_scene()
    crowd = [grid(70), grid(70, shift=2.0)]
    kp, det, fr = pack([pad_joints(crowd, SCENE_K), video, [], video[:7]])
    n = kp.shape[0]
    a = run(be, kp, det, fr)
    b = run(be, kp, det, fr)
    assert a[0] == 0 and b[0] == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))
    assert (a[1][:n] != SENTINEL_I).all() and (a[2][:n] != SENTINEL_F).all() and (a[3] != SENTINEL_I).all()
    assert (a[1][n:] == SENTINEL_I).all() and (a[2][n:] == SENTINEL_F).all()
    c = run(be, kp, det, fr, want_sim=False)
    assert c[0] == 0 and c[2] is None and c[1].tobytes() == a[1].tobytes() and c[3].tobytes() == a[3].tobytes()
    rt, _, rv = ref_track(kp, det, fr, **RULE)
    assert np.array_equal(a[1][:n], rt) and np.array_equal(a[3], rv)


def case_arguments(be):
    """Every DYB_ERR_ARG row leaves the sentinel outputs untouched; n = 0 is legal."""
    video, _ = make_scene()
    kp, det, fr = pack([video[:4], video[4:6]])
    for kw in (dict(null=("kp",)), dict(null=("track",)), dict(null=("det",)), dict(null=("fr",)), dict(null=("video",)), dict(K=0), dict(K=33),
               dict(kappa=0.0), dict(kappa=-0.1), dict(s_min=0.0), dict(s_min=-0.5), dict(s_min=1.5), dict(max_age=-1), dict(min_common=0),
               dict(c_min=float("nan")), dict(c_min=float("inf")), dict(kappa=float("inf")), dict(kappa=float("nan")), dict(s_min=float("nan")),
               dict(n=-1), dict(F=-1), dict(V=0), dict(V=-1)):
        rc, tr, sim, vid = run(be, kp, det, fr, **kw)
        assert rc == ERR_ARG, kw
        assert (tr == SENTINEL_I).all() and (sim == SENTINEL_F).all() and (vid == SENTINEL_I).all(), kw
    rc, tr, sim, vid = run(be, kp[:0], np.zeros(3, np.int32), np.array([0, 2], np.int32), null=("kp", "track", "sim"))
    assert rc == 0 and vid.tolist() == [[0, 0, 0, 0]]
    rc, tr, sim, vid = run(be, kp[:0], np.zeros(1, np.int32), np.array([0, 0], np.int32))                     # no frames at all
    assert rc == 0 and vid.tolist() == [[0, 0, 0, 0]] and (tr == SENTINEL_I).all()
    rc, tr, sim, vid = run(be, kp, det, fr, s_min=1.0)                                                           # the closed end of (0, 1]
    assert rc == 0
