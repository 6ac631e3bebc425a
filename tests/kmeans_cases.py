"""Cases of the k-means kernels (csrc/kmeans.hip) through the C ABI, for either backend (tests/backends.py), and the fp64 restatements
they are checked against: cosines, argmax with ties to the lowest index, member means and the Lloyd loop with its reseed rule, all in
NumPy fp64 and none of it a call into the library.  Bounds are derived from the number of fp32 roundings (gamma_n = n u / (1 - n u),
u = 2^-24), not tuned."""
import numpy as np

from retrieval_cases import MARGIN, philox4x32_10

U = 2.0 ** -24
NS = (1, 31, 64, 65, 130, 300)              # the edges of a 64- or 128-row tile, more than one workgroup
KS = (1, 3, 32, 33, 67, 130)                # the edges of the 32-column tiles, one / two / four tiles per pass, two passes
DS = (64, 2048)
UPDATE_EXTRA = ((1200, 3, 64),              # 19 row chunks: more than the eight groups of the update's second launch
                (2500, 130, 64))            # K > 32 with a chunk of 2112 rows: two blocks of the member list, then a second chunk
PAD = 8                                     # floats of padding in the padded-stride cases (the pitch stays a multiple of 16 bytes)


def gamma(n):
    return n * U / (1.0 - n * U)


def make_centres(K, D, rng):
    return rng.normal(0, 1, (K, D)).astype(np.float32)


def make_rows(centers, targets, rng):
    """retrieval_cases.make_rows for any D: x = a * centre_target + a * noise, cosine ~ 0.7 to the target, ~ N(0, 1 / D) to the others"""
    D = centers.shape[1]
    a = rng.uniform(0.5, 2.0, len(targets))
    return np.stack([(a[i] * centers[t] + a[i] * rng.normal(0, 1, D)).astype(np.float32) for i, t in enumerate(targets)])


def assign_inputs(N, K, D):
    """(x [N][D], centres [K][D], targets) of the assign case of this shape: seeded by the shape"""
    rng = np.random.default_rng(7919 * N + 31 * K + D)
    centers = make_centres(K, D, rng)
    targets = rng.integers(0, K, N)
    return make_rows(centers, targets, rng), centers, targets


def cosines64(x, centers, x_inv=None, c_inv=None):
    """[N][K] fp64 cosines; the inverse norms are the fp64 ones unless the (fp32) values a kernel was given are passed in"""
    x64, c64 = x.astype(np.float64), centers.astype(np.float64)
    xi = 1.0 / np.maximum(np.sqrt((x64 ** 2).sum(1)), 1e-8) if x_inv is None else x_inv.astype(np.float64)
    ci = 1.0 / np.maximum(np.sqrt((c64 ** 2).sum(1)), 1e-8) if c_inv is None else c_inv.astype(np.float64)
    return (x64 @ c64.T) * xi[:, None] * ci[None, :]


def argmax_margin(cos):
    """-> (argmax with ties to the lowest index [N], winning value [N], gap to the best OTHER value [N] - inf where there is none)"""
    best = cos.max(1)
    arg = np.array([int(np.flatnonzero(r == b)[0]) for r, b in zip(cos, best)])
    gap = np.full(len(cos), np.inf)
    for i, r in enumerate(cos):
        o = r[r < best[i]]
        if len(o):
            gap[i] = best[i] - o.max()
    return arg, best, gap


# ------------------------------------------------------------------------------------------------------------------ library calls
def padded(be, x, pad):
    """device copy of x with `pad` floats of NaN after every row -> (buffer, stride in bytes)"""
    N, D = x.shape
    h = np.full((N, D + pad), np.nan, np.float32)
    h[:, :D] = x
    return be.dev(h), (D + pad) * 4


def run_inv_norm(be, x, pad=0):
    N, D = x.shape
    buf, stride = padded(be, x, pad)
    out = be.dev(np.full(N, -7.0, np.float32))
    rc = be.lib.dyb_rows_inv_norm(be.ptr(buf), stride, N, D, be.ptr(out), be.stream)
    assert rc == 0
    return be.host(out)


def run_assign(be, x, centers, prev, pad=0, x_inv=None, c_inv=None):
    """-> dict(rc, assign, best, changed, counts, objective, x_inv, c_inv); the inverse norms come from dyb_rows_inv_norm unless given"""
    N, D = x.shape
    K = centers.shape[0]
    x_inv = run_inv_norm(be, x) if x_inv is None else x_inv
    c_inv = run_inv_norm(be, centers) if c_inv is None else c_inv
    buf, stride = padded(be, x, pad)
    assign = be.dev(np.asarray(prev, np.int32), np.int32)
    best = be.dev(np.full(N, -7.0, np.float32))
    changed = be.dev(np.array([-7], np.int32), np.int32)
    counts = be.dev(np.full(K, -7, np.int32), np.int32)
    wsb = int(be.lib.dyb_kmeans_assign_workspace_bytes(N, D, K))
    assert wsb == 8 * ((N + 127) // 128)
    ws = be.dev(np.zeros(wsb // 4, np.int32), np.int32)
    rc = be.lib.dyb_kmeans_assign(be.ptr(buf), stride, be.ptr(be.dev(x_inv)), N, D, be.ptr(be.dev(centers)), be.ptr(be.dev(c_inv)), K,
                                  be.ptr(assign), be.ptr(best), be.ptr(changed), be.ptr(counts), be.ptr(ws), wsb, be.stream)
    parts = be.host(ws).view(np.float64)
    return dict(rc=rc, assign=be.host(assign), best=be.host(best), changed=int(be.host(changed)[0]), counts=be.host(counts),
                parts=parts, x_inv=x_inv, c_inv=c_inv)


def run_update(be, x, x_inv, assign, counts, centers0, pad=0):
    N, D = x.shape
    K = centers0.shape[0]
    buf, stride = padded(be, x, pad)
    centers = be.dev(centers0)
    wsb = int(be.lib.dyb_kmeans_update_workspace_bytes(N, D, K))
    ws = be.dev(np.full(max(wsb // 4, 1), np.nan, np.float32))
    rc = be.lib.dyb_kmeans_update(be.ptr(buf), stride, be.ptr(be.dev(x_inv)), N, D, be.ptr(be.dev(assign, np.int32)),
                                  be.ptr(be.dev(counts, np.int32)), K, be.ptr(centers), be.ptr(ws), wsb, be.stream)
    return rc, be.host(centers)


# ------------------------------------------------------------------------------------------------------------------ cases
def check_inv_norm(be, N, D, pad=0):
    rng = np.random.default_rng(N + D)
    x = (rng.normal(0, 1, (N, D)) * rng.uniform(0.01, 30.0, (N, 1))).astype(np.float32)
    x[0] = 0.0                                                              # the clamp: 1 / 1e-8
    got = run_inv_norm(be, x, pad).astype(np.float64)
    want = 1.0 / np.maximum(np.sqrt((x.astype(np.float64) ** 2).sum(1)), 1e-8)
    # D squares and at most D additions per element (any order), the square root halves the relative error and adds one rounding,
    # the division another, the clamp constant is an fp32 number: gamma_(D + 3) relative covers it
    assert (np.abs(got - want) <= gamma(D + 3) * want).all(), float(np.abs(got / want - 1).max())


def check_assign(be, N, K, D, pad=0):
    x, centers, _ = assign_inputs(N, K, D)
    rng = np.random.default_rng(N * K + D)
    r = run_assign(be, x, centers, np.full(N, -1, np.int32), pad=pad)
    assert r["rc"] == 0
    cos = cosines64(x, centers, r["x_inv"], r["c_inv"])
    arg, best, _ = argmax_margin(cos)
    assert np.array_equal(r["assign"], arg)
    assert np.array_equal(r["counts"], np.bincount(arg, minlength=K)) and r["changed"] == N
    # D products and D additions in one chain of fused multiply-adds (D roundings), then the two inverse norms: gamma_(D + 2)
    absdot = np.abs(x.astype(np.float64)) @ np.abs(centers.astype(np.float64)).T
    bound = gamma(D + 2) * absdot[np.arange(N), arg] * r["x_inv"].astype(np.float64) * r["c_inv"][arg].astype(np.float64)
    assert (np.abs(r["best"].astype(np.float64) - best) <= bound).all()
    # the objective partials: fp64 sums of the fp32 `best` per 128 rows, in row order - exact up to fp64 rounding of <= 128 terms
    for w, p in enumerate(r["parts"]):
        seg = r["best"][128 * w:128 * (w + 1)].astype(np.float64)
        assert abs(p - seg.sum()) <= 128 * 2.0 ** -53 * np.abs(seg).sum()
    # `changed` against a previous assignment that is partly right, partly wrong, partly unset
    prev = arg.copy()
    flip = rng.random(N) < 0.4
    prev[flip] = rng.integers(-1, K, int(flip.sum()))
    r2 = run_assign(be, x, centers, prev, pad=pad, x_inv=r["x_inv"], c_inv=r["c_inv"])
    assert r2["rc"] == 0 and r2["changed"] == int((prev != arg).sum())
    assert r2["assign"].tobytes() == r["assign"].tobytes() and r2["best"].tobytes() == r["best"].tobytes()
    assert np.array_equal(r2["counts"], r["counts"])


def check_assign_tie(be, D):
    """identical centres in one tile, in two tiles of a pass and in two passes: the lower index, for rows aimed at the higher one"""
    K = 140
    rng = np.random.default_rng(77 + D)
    centers = make_centres(K, D, rng)
    pairs = ((2, 5), (3, 40), (7, 135))
    for lo, hi in pairs:
        centers[hi] = centers[lo]
    targets = [hi for _, hi in pairs for _ in range(3)]
    x = make_rows(centers, targets, rng)
    r = run_assign(be, x, centers, np.full(len(targets), -1, np.int32))
    arg, _, gap = argmax_margin(cosines64(x, centers))
    assert r["rc"] == 0 and (gap >= MARGIN).all()
    assert list(arg) == [lo for lo, _ in pairs for _ in range(3)] and np.array_equal(r["assign"], arg)


def check_assign_errors(be):
    rng = np.random.default_rng(5)
    N, K, D = 10, 4, 64
    x, centers = rng.normal(0, 1, (N, D)).astype(np.float32), make_centres(K, D, rng)
    xi, ci = run_inv_norm(be, x), run_inv_norm(be, centers)
    lib = be.lib
    assign = be.dev(np.full(N, -7, np.int32), np.int32)
    best = be.dev(np.full(N, -7.0, np.float32))
    changed = be.dev(np.array([-7], np.int32), np.int32)
    counts = be.dev(np.full(K, -7, np.int32), np.int32)
    ws = be.dev(np.full(64, -7, np.int32), np.int32)
    bx, bc, bxi, bci = be.dev(x), be.dev(np.concatenate([centers] * 300)[:1025]), be.dev(xi), be.dev(np.resize(ci, 1025))
    p = be.ptr

    def call(x_=bx, stride=D * 4, xi_=bxi, N_=N, D_=D, c_=bc, ci_=bci, K_=K, a_=assign, b_=best, ch_=changed, cn_=counts, ws_=ws, wsb=256):
        return lib.dyb_kmeans_assign(p(x_), stride, p(xi_), N_, D_, p(c_), p(ci_), K_, p(a_), p(b_), p(ch_), p(cn_), p(ws_), wsb, be.stream)

    for kw in (dict(x_=None), dict(xi_=None), dict(c_=None), dict(ci_=None), dict(a_=None), dict(b_=None), dict(ch_=None), dict(cn_=None),
               dict(ws_=None), dict(N_=0), dict(K_=0), dict(stride=D * 4 - 16), dict(stride=D * 4 + 4)):
        assert call(**kw) == -1, kw
    assert call(D_=48, stride=48 * 4) == -3 and call(D_=0) == -1
    assert call(K_=1025) == -3
    assert call(wsb=7) == -4
    assert lib.dyb_rows_inv_norm(None, D * 4, N, D, p(best), be.stream) == -1
    assert lib.dyb_rows_inv_norm(p(bx), D * 4, N, 48, p(best), be.stream) == -3
    assert lib.dyb_kmeans_assign_workspace_bytes(N, 48, K) == 0 and lib.dyb_kmeans_update_workspace_bytes(N, D, 1025) == 0
    # the update's argument checks
    uws = be.dev(np.full(N * K * D, -7.0, np.float32))
    cen = be.dev(np.full((K, D), -7.0, np.float32))
    good = be.dev(np.zeros(N, np.int32), np.int32)

    def upd(x_=bx, xi_=bxi, D_=D, a_=good, cn_=counts, K_=K, c_=cen, ws_=uws, wsb=N * K * D * 4):
        return lib.dyb_kmeans_update(p(x_), D * 4, p(xi_), N, D_, p(a_), p(cn_), K_, p(c_), p(ws_), wsb, be.stream)

    for kw in (dict(x_=None), dict(xi_=None), dict(a_=None), dict(cn_=None), dict(c_=None), dict(ws_=None), dict(K_=0)):
        assert upd(**kw) == -1, kw
    assert upd(D_=48) == -3 and upd(K_=1025) == -3
    assert upd(wsb=int(lib.dyb_kmeans_update_workspace_bytes(N, D, K)) - 4) == -4
    # nothing was written by any of the refused calls
    for buf in (assign, changed, counts, ws):
        assert (be.host(buf) == -7).all()
    assert (be.host(best) == -7.0).all() and (be.host(cen) == -7.0).all() and (be.host(uws) == -7.0).all()


def update_assignment(N, K, mode, rng):
    """random: a random assignment with cluster K - 1 (K > 1) emptied into cluster 0 and, for K > 2, a second empty cluster 1;
    one: every row in cluster K // 2"""
    if mode == "one":
        return np.full(N, K // 2, np.int32)
    a = rng.integers(0, K, N).astype(np.int32)
    if K > 1:
        a[a == K - 1] = 0
    if K > 2:
        a[a == 1] = 0
    return a


def check_update(be, N, K, D, mode, pad=0):
    rng = np.random.default_rng(104729 * N + 13 * K + D + (mode == "one"))
    x = (rng.normal(0, 1, (N, D)) * rng.uniform(0.2, 5.0, (N, 1))).astype(np.float32)
    x_inv = run_inv_norm(be, x)
    a = update_assignment(N, K, mode, rng)
    counts = np.bincount(a, minlength=K).astype(np.int32)
    assert K == 1 or (counts == 0).any()
    centers0 = rng.normal(0, 1, (K, D)).astype(np.float32)
    rc, got = run_update(be, x, x_inv, a, counts, centers0, pad=pad)
    assert rc == 0
    # the reference takes the device's fp32 inverse norms as given: what is checked is the mean, with one rounding for the product
    # x * inv, at most n_k - 1 for the additions (adding a zero partial is exact) and one for the division: gamma_(n_k + 2)
    xn = x.astype(np.float64) * x_inv.astype(np.float64)[:, None]
    for k in range(K):
        if counts[k] == 0:
            assert got[k].tobytes() == centers0[k].tobytes(), k
            continue
        m = a == k
        want = xn[m].sum(0) / counts[k]
        bound = gamma(int(counts[k]) + 2) * np.abs(xn[m]).sum(0) / counts[k]
        assert (np.abs(got[k].astype(np.float64) - want) <= bound).all(), (k, counts[k])
    rc, again = run_update(be, x, x_inv, a, counts, centers0, pad=pad)
    assert rc == 0 and again.tobytes() == got.tobytes()
    return got


# ------------------------------------------------------------------------------------------------------------------ Lloyd in fp64
def lloyd64(x, init, max_iter=100):
    """The loop of retrieval_index.lloyd restated: fp64 cosines and means, ties to the lowest index, the same stop and reseed rules.
    -> dict(assign per iteration (after reseeds), centers, iterations, reseeds, margins): margins collects the gap of every decision
    the run took - each row's best against its second-best cosine at every assign, and each reseed's row against the runner-up."""
    x64 = x.astype(np.float64)
    xn = x64 / np.maximum(np.sqrt((x64 ** 2).sum(1)), 1e-8)[:, None]
    N, K = len(x), len(init)
    centers = init.astype(np.float64).copy()
    assign = np.full(N, -1)
    out = dict(assign=[], iterations=0, reseeds=0, margins=[], reseed_margins=[])
    for _ in range(max_iter):
        cn = centers / np.maximum(np.sqrt((centers ** 2).sum(1)), 1e-8)[:, None]
        arg, best, gap = argmax_margin(xn @ cn.T)
        out["margins"].append(float(gap.min()))
        changed = int((arg != assign).sum())
        assign = arg.copy()
        counts = np.bincount(assign, minlength=K)
        out["iterations"] += 1
        empty = [k for k in range(K) if counts[k] == 0]
        taken = set()
        for k in empty:
            cand = [i for i in np.lexsort((np.arange(N), best)) if i not in taken and counts[assign[i]] > 1]
            if not cand:
                break
            row = int(cand[0])
            if len(cand) > 1:
                out["reseed_margins"].append(float(best[cand[1]] - best[row]))
            taken.add(row)
            counts[assign[row]] -= 1
            assign[row] = k
            counts[k] = 1
            out["reseeds"] += 1
        out["assign"].append(assign.copy())
        if changed == 0 and not empty:
            break
        for k in range(K):
            if counts[k]:
                centers[k] = xn[assign == k].sum(0) / counts[k]
    out["centers"] = centers
    return out


BLOBS, BLOB_N, BLOB_D = 5, 300, 2048


def blob_data():
    """Five well-separated blobs on the sphere, built so that every decision of the three runs below has a wide margin: random unit
    directions e_b (nearly orthogonal in 2048 dimensions), row = scale * (u + noise), |noise| ~ 0.25 (cosine ~ 0.94 inside a blob).
    Blob 0 has two halves u = e_0 +- 0.3 v (two seeds in it split it cleanly); blob 4 leans towards blob 1 (u = e_4 + 0.3 e_1) and
    blob 2 towards blob 3 (u = e_2 + 0.3 e_3), so that an unseeded blob goes to ONE known centre; row 2 (of blob 2) leans only half
    as far (0.15): the row of lowest `best` once blob 2 has lost its centre, by a wide gap.  -> (x [300][2048] fp32, blob [300])"""
    rng = np.random.default_rng(2024)
    e = rng.normal(0, 1, (BLOBS + 1, BLOB_D))
    e /= np.sqrt((e ** 2).sum(1))[:, None]
    blob = np.arange(BLOB_N) % BLOBS
    x = np.empty((BLOB_N, BLOB_D), np.float32)
    for i in range(BLOB_N):
        b = blob[i]
        u = e[b].copy()
        if b == 0:
            u += (0.3 if (i // BLOBS) % 2 == 0 else -0.3) * e[BLOBS]
        elif b == 4:
            u += 0.3 * e[1]
        elif b == 2:
            u += (0.15 if i == 2 else 0.3) * e[3]
        x[i] = (rng.uniform(0.5, 3.0) * (u + rng.normal(0, 0.25 / np.sqrt(BLOB_D), BLOB_D))).astype(np.float32)
    return x, blob


def blob_inits():
    """rows 0 and 5 are the two halves of blob 0, rows 1, 7, 3, 4 lie in blobs 1, 2, 3, 4 (7, not the odd row 2)"""
    x, _ = blob_data()
    away = x[[0, 1, 7, 3, 4]].copy()
    away[2] = -x[[0, 1, 7, 3, 4]].astype(np.float64).sum(0).astype(np.float32)   # negative cosine to every row: empty after the first assign
    return {"one_per_blob": x[[0, 1, 7, 3, 4]].copy(), "two_in_one": x[[0, 5, 1, 7, 3]].copy(), "away": away}


def philox_init_rows(N, K, seed):
    """restatement of the documented rule of kmeans(init=None): counter (j, 0, 0, 1), key (seed lo, seed hi), r = j + mulhi32(w, N - j)"""
    idx = list(range(N))
    for j in range(K):
        w = philox4x32_10([j, 0, 0, 1], [seed & 0xffffffff, seed >> 32])[0]
        r = j + ((w * (N - j)) >> 32)
        idx[j], idx[r] = idx[r], idx[j]
    return idx[:K]


def philox_select(assign, K, per_cluster, seed):
    """restatement of select_members(mode='random'): counter (j, 0, k, 2)"""
    out = []
    for k in range(K):
        m = [int(i) for i in np.flatnonzero(np.asarray(assign) == k)]
        take = min(per_cluster, len(m))
        for j in range(take):
            w = philox4x32_10([j, 0, k, 2], [seed & 0xffffffff, seed >> 32])[0]
            r = j + ((w * (len(m) - j)) >> 32)
            m[j], m[r] = m[r], m[j]
        out.append(m[:take])
    return out
