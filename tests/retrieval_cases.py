"""Cases of the exemplar bank's two kernels (csrc/retrieval.hip) through the C ABI, for either backend (tests/backends.py).
The check is independent of the library: cosines recomputed in fp64 by NumPy, a Philox-4x32-10 of its own, ties to the lowest index."""
import ctypes

import numpy as np

D = 2048
MARGIN = 1e-3                  # fp64 gap best - second best cosine every generated row must have (asserted): the fp32 summation order of the
#                                kernel (error ~ 2048 * 2^-24 * |x||c| relative ~ 1e-4 at worst, typically 1e-6) then cannot decide the argmax
M32 = 0xffffffff


def philox4x32_10(c, k):
    c, k = [int(v) & M32 for v in c], [int(v) & M32 for v in k]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k[0]) & M32, p1 & M32, ((p0 >> 32) ^ c[3] ^ k[1]) & M32, p0 & M32]
        k = [(k[0] + 0x9E3779B9) & M32, (k[1] + 0xBB67AE85) & M32]
    return c


def expected_pick(x, centers, inv_norm, index, draw, seed, sample=0):
    """-> (cluster, item, margin): argmax of the fp64 cosine (lowest index on a tie), the member the draw takes, and the gap to the best
    cosine of any OTHER value (identical rows share a value: their tie is settled by index, not by rounding)."""
    x64 = x.astype(np.float64)
    cos = (centers.astype(np.float64) @ x64) * inv_norm.astype(np.float64) / max(np.sqrt(x64 @ x64), 1e-300)
    c = int(np.flatnonzero(cos == cos.max())[0])
    others = cos[cos < cos.max()]
    margin = float(cos.max() - others.max()) if len(others) else np.inf
    n = len(index[c])
    if n == 0:
        return c, -1, margin
    w = philox4x32_10([draw & M32, (draw >> 32) & M32, sample, 0], [seed & M32, (seed >> 32) & M32])[0]
    return c, int(index[c][(w * n) >> 32]), margin


def make_bank(K, rng, sizes=(1, 4, 7), empty=()):
    centers = rng.normal(0, 1, (K, D)).astype(np.float32)
    inv = (1.0 / np.sqrt((centers.astype(np.float64) ** 2).sum(1))).astype(np.float32)
    ns = [0 if k in empty else sizes[k % len(sizes)] for k in range(K)]
    perm = rng.permutation(sum(ns))
    index, at = [], 0
    for n in ns:
        index.append([int(i) for i in perm[at:at + n]])
        at += n
    return centers, inv, index


def make_rows(centers, targets, rng):
    """x = a * centre_target + noise: cosine ~ 0.7 to the target, ~ N(0, 1 / 2048) to every other random centre"""
    a = rng.uniform(0.5, 2.0, len(targets))
    return np.stack([(a[i] * centers[t] + a[i] * rng.normal(0, 1, D)).astype(np.float32) for i, t in enumerate(targets)])


def csr(index):
    ptr = np.zeros(len(index) + 1, np.int32)
    ptr[1:] = np.cumsum([len(m) for m in index])
    flat = [i for m in index for i in m]
    return ptr, np.array(flat if flat else [0], np.int32)


def run_select(be, feats, nrep, active, centers, inv, index, draws, seed, chunk=0, cap=4, check=1, K=None, n_items=None):
    """feats: [nrep][2048] (rows of inactive replicas NaN) -> (rc, picks [nrep][cap][2])"""
    lib = be.lib
    K = centers.shape[0] if K is None else K
    ptr, idx = csr(index)
    n_items = max(int(idx.max()) + 1, 1) if n_items is None else n_items
    picks = be.dev(np.full((nrep, cap, 2), -7, np.int32), np.int32)
    wsb = max(int(lib.dyb_retrieve_workspace_bytes(len(active), max(K, 1), chunk)), 256)
    ws = be.dev(np.zeros(wsb // 4 + 4, np.int32), np.int32)
    rows = (ctypes.c_int * len(active))(*active)
    dr = (ctypes.c_ulonglong * 64)(*([int(d) for d in draws] + [0] * (64 - len(draws))))
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)
    rc = lib.dyb_retrieve_select(be.ptr(be.dev(feats)), D * 4, vp(rows), len(active), be.ptr(be.dev(centers)), be.ptr(be.dev(inv)), K,
                                 be.ptr(be.dev(ptr, np.int32)), be.ptr(be.dev(idx, np.int32)), len(idx), n_items, vp(dr), seed, 0,
                                 be.ptr(picks), cap * 8, cap, chunk, check, be.ptr(ws), wsb, be.stream)
    return rc, be.host(picks)


REPLICA_SETS = {"one": (1, [0]), "sparse": (5, [1, 4]), "all64": (64, list(range(64)))}
DRAWS = (0, 1, (1 << 32) + 3)


def case_select(be, K, reps, chunk):
    nrep, active = REPLICA_SETS[reps]
    rng = np.random.default_rng(1000 * K + nrep)
    centers, inv, index = make_bank(K, rng)
    targets = {r: int(rng.integers(0, K)) for r in active}
    feats = np.full((nrep, D), np.nan, np.float32)
    feats[active] = make_rows(centers, [targets[r] for r in active], rng)
    draws = [DRAWS[r % 3] for r in range(nrep)]
    seed = (0x9abc << 32) | 0x1234567
    rc, picks = run_select(be, feats, nrep, active, centers, inv, index, draws, seed, chunk=chunk)
    assert rc == 0
    for r in range(nrep):
        if r not in active:
            assert (picks[r] == -7).all(), r                               # an inactive replica's log is not touched
            continue
        c, item, margin = expected_pick(feats[r], centers, inv, index, draws[r], seed)
        assert K == 1 or margin >= MARGIN, (r, margin)                       # (asserted, not skipped: the generator guarantees it)
        assert c == targets[r]
        row = draws[r] % 4
        assert tuple(picks[r, row]) == (c, item), (r, picks[r], c, item)
        assert (np.delete(picks[r], row, 0) == -7).all()
    return picks


def case_tie_lowest_index(be, chunk):
    rng = np.random.default_rng(77)
    K = 40
    centers, inv, index = make_bank(K, rng)
    centers[21] = centers[6]                                                 # 6 and 21 fall into different chunks for chunk 16 and 5
    inv[21] = inv[6]
    feats = make_rows(centers, [21], rng)
    rc, picks = run_select(be, feats, 1, [0], centers, inv, index, [2], 5, chunk=chunk)
    c, item, margin = expected_pick(feats[0], centers, inv, index, 2, 5)
    assert rc == 0 and c == 6 and margin >= MARGIN and tuple(picks[0, 2]) == (6, item)


def case_select_errors(be):
    rng = np.random.default_rng(5)
    centers, inv, index = make_bank(9, rng, empty=(4,))
    feats = make_rows(centers, [4, 3], rng)
    # the nearest cluster of row 0 is empty: DYB_ERR_ARG from the checking form, item -1 in the log either way; row 1 is served
    rc, picks = run_select(be, feats, 2, [0, 1], centers, inv, index, [0, 0], 1, n_items=64)
    assert rc == -1 and tuple(picks[0, 0]) == (4, -1) and picks[1, 0, 0] == 3 and picks[1, 0, 1] >= 0
    rc, picks = run_select(be, feats, 2, [0, 1], centers, inv, index, [0, 0], 1, check=0, n_items=64)
    assert rc == 0 and tuple(picks[0, 0]) == (4, -1)
    rc, _ = run_select(be, feats, 2, [0, 1], centers, inv, index, [0, 0], 1, K=0)
    assert rc == -1
    rc, _ = run_select(be, feats[:1], 1, [64], centers, inv, index, [0], 1)       # a replica index outside 0 .. 63
    assert rc == -1


SIZES = dict(img=3 * 224 * 224, keypoints=147, pose=72, betas=10, pose_3d=96)


def case_gather(be):
    rng = np.random.default_rng(9)
    N, nrep, cap = 12, 6, 3
    bank = {k: rng.normal(0, 1, (N, n)).astype(np.float32) for k, n in SIZES.items()}
    active, draws = [0, 2, 5], [4, 0, 2, 0, 0, 7]                             # rows 1, 2, 1 of the logs
    picks = np.full((nrep, cap, 2), -1, np.int32)
    want = {0: 7, 2: 7, 5: 11}                                                # repeats across replicas, the last item
    for r, item in want.items():
        picks[r, draws[r] % cap] = (1, item)
    picks[3, 0] = (0, 3)                                                      # an inactive replica with a valid pick: still untouched
    outs = {k: be.dev(np.full((nrep, n), 123.5, np.float32)) for k, n in SIZES.items()}
    dst = (ctypes.c_void_p * 5)(*[be.ptr(outs[k]) for k in SIZES])
    strides = (ctypes.c_size_t * 5)(*[4 * n for n in SIZES.values()])
    rows = (ctypes.c_int * 3)(*active)
    dr = (ctypes.c_ulonglong * 64)(*(draws + [0] * 58))
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)
    dbank = {k: be.dev(v) for k, v in bank.items()}
    rc = be.lib.dyb_exemplar_gather(be.ptr(be.dev(picks, np.int32)), cap * 8, cap, vp(rows), 3, vp(dr), *[be.ptr(dbank[k]) for k in SIZES], N,
                                    vp(dst), vp(strides), be.stream)
    assert rc == 0
    for k in SIZES:
        got = be.host(outs[k])
        for r in range(nrep):
            if r in want:
                assert got[r].tobytes() == bank[k][want[r]].tobytes(), (k, r)
            else:
                assert (got[r] == 123.5).all(), (k, r)
    # a logged item outside the bank copies nothing
    picks[0, draws[0] % cap] = (1, N)
    outs2 = {k: be.dev(np.full((nrep, n), 123.5, np.float32)) for k, n in SIZES.items()}
    dst2 = (ctypes.c_void_p * 5)(*[be.ptr(outs2[k]) for k in SIZES])
    rows1 = (ctypes.c_int * 1)(0)
    rc = be.lib.dyb_exemplar_gather(be.ptr(be.dev(picks, np.int32)), cap * 8, cap, vp(rows1), 1, vp(dr), *[be.ptr(dbank[k]) for k in SIZES], N,
                                    vp(dst2), vp(strides), be.stream)
    assert rc == 0 and all((be.host(outs2[k]) == 123.5).all() for k in SIZES)
