"""numpy restatement of csrc/validity.hip's definitions (include/shotvae_hip.h: sv_sil_scan, sv_sil_finish, sv_cluster_spread) and of
shot_vae_amd/validity.py, in two forms: a DENSE one in float64 (the distance matrix from direct differences, numpy's own sums) and one
that walks columns, tiles, segments, partial states and merge trees IN THE KERNEL'S ORDER with the kernel's fp32 pair values
(tests/_twosample_ref.pair_values32: the exact fmaf emulation).  tests/test_validity_cpu.py pins the dense form to scikit-learn; the GPU
tests compare the kernels with both and take their allowances from here, never from a GPU result."""
import numpy as np

from tests._twosample_ref import RBF, butterfly16, pair_values, pair_values32

EUCLID, SQEUCLID = 0, 1
METRIC = {"euclid": EUCLID, "sqeuclid": SQEUCLID}
TILE = 64


# ---------------------------------------------------------------------------------------------- distances
def distances(metric, q, g, fp32=False):
    """float64 [Q, N]: |q_i - g_j| (EUCLID) or |q_i - g_j|^2 (SQEUCLID) from the differences themselves in float64, or (fp32) from the
    kernel's fp32 pair values with the fp32 correctly rounded root"""
    with np.errstate(invalid="ignore", over="ignore"):
        if fp32:
            v = pair_values32(RBF, q, g)
            return (np.sqrt(v) if metric == EUCLID else v).astype(np.float64)      # numpy's float32 sqrt: correctly rounded
        v = pair_values(RBF, q, g)
        return np.sqrt(v) if metric == EUCLID else v


def clip_seg(seg, N):
    return np.clip(np.asarray(seg, dtype=np.int64), 0, N)


def grouped(x, labels, k):
    """(g, key sorted, order, seg): the rows of x grouped by a STABLE sort of their cluster; a label outside [0, k) or a row that is not
    finite gets the key k and sorts behind seg[k]"""
    x, labels = np.asarray(x, dtype=np.float64), np.asarray(labels, dtype=np.int64)
    key = np.where((labels >= 0) & (labels < k) & np.isfinite(x).all(axis=1), labels, k)
    order = np.argsort(key, kind="stable")
    seg = np.searchsorted(key[order], np.arange(k + 1))
    return x[order], key[order], order, seg.astype(np.int64)


# ---------------------------------------------------------------------------------------------- the dense form
def min_keep_nan(m, v):
    """the running minimum m = (v < m || v != v) ? v : m, elementwise"""
    with np.errstate(invalid="ignore"):
        return np.where((v < m) | np.isnan(v), v, m)


def silhouette_of(ta, tb, q_label, seg, K, N):
    """(s, a, b) from a row's own sum ta and its smallest other mean tb: sv_sil_finish's per-row rule, every operation rounded once"""
    q_label, seg = np.asarray(q_label, dtype=np.int64), clip_seg(seg, N)
    known = (q_label >= 0) & (q_label < K)
    lab = np.where(known, q_label, 0)
    n_own = np.where(known, seg[lab + 1] - seg[lab], 0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        a = np.where(n_own > 1, ta / np.maximum(n_own - 1, 1).astype(np.float64), np.where(n_own == 1, 0.0, np.nan))
        ok = (n_own >= 1) & ~np.isnan(a) & ~np.isnan(tb) & (tb < np.inf)
        hi = np.where(a > tb, a, tb)
        s = np.where(ok, np.where((n_own == 1) | (hi == 0.0), 0.0, (tb - a) / np.where(hi == 0.0, 1.0, hi)), np.nan)
    return s, a, np.asarray(tb, dtype=np.float64).copy()


def dense(dist, q_label, seg, K):
    """(s, a, b) float64 [Q] from the distance matrix [Q, N] of queries against a grouped gallery: numpy's own sums"""
    Q, N = dist.shape
    q_label, sg = np.asarray(q_label, dtype=np.int64), clip_seg(seg, N)
    ta, tb = np.zeros(Q), np.full(Q, np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(K):
            lo, hi = int(sg[c]), int(sg[c + 1])
            if hi <= lo:
                continue
            t = dist[:, lo:hi].sum(axis=1)
            mine = q_label == c
            ta = np.where(mine, t, ta)
            tb = np.where(mine, tb, min_keep_nan(tb, t / float(hi - lo)))
    return silhouette_of(ta, tb, q_label, seg, K, N)


def silhouette_samples(x, labels, k, metric=EUCLID, fp32=False):
    """float64 [n] in the caller's order: the package's silhouette_samples, dense"""
    g, key, order, seg = grouped(x, labels, k)
    with np.errstate(invalid="ignore"):
        s_sorted = dense(distances(metric, g, g, fp32), key, seg, k)[0]
    s = np.empty(len(order))
    s[order] = s_sorted
    return s


def allowance(metric, q, q_label, g, seg, K):
    """the 8x rule for one case: 8 x the largest error of the fp32 restatement (the kernel's fp32 pair values and roots, float64 sums
    and divisions) against the float64 one, for s, a and b separately.  -> ((tol_s, tol_a, tol_b), (err_s, err_a, err_b))"""
    ref = dense(distances(metric, q, g), q_label, seg, K)
    f32 = dense(distances(metric, q, g, fp32=True), q_label, seg, K)
    errs = []
    for r, f in zip(ref, f32):
        fin = np.isfinite(r) & np.isfinite(f)
        errs.append(float(np.max(np.abs(f - r)[fin])) if fin.any() else 0.0)
    return tuple(8.0 * e for e in errs), tuple(errs)


# ---------------------------------------------------------------------------------------------- the kernel's order
def ordered_parts(metric, q, q_label, g, seg, K, P, V=None):
    """(part_a, part_b) float64 [P, Q] as sv_sil_scan leaves them: state p walks the non-empty clusters p, p + P, ..; a cluster's rows in
    tiles of 64 from its first row; thread tx of a row's 16 adds the columns 4 tx .. 4 tx + 3 of every tile in order from 0.0; at the
    end of the cluster the shares meet in the butterfly and the total is the row's own sum or enters its running minimum, divided once
    by the cluster's size.  V: the distances [Q, N] to add (default: the kernel's fp32 values as float64)"""
    V = distances(metric, q, g, fp32=True) if V is None else np.asarray(V, dtype=np.float64)
    Q, N = V.shape
    q_label, sg = np.asarray(q_label, dtype=np.int64), clip_seg(seg, N)
    part_a, part_b = np.zeros((P, Q)), np.full((P, Q), np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        for p in range(P):
            for c in range(p, K, P):
                lo, hi = int(sg[c]), int(sg[c + 1])
                if hi <= lo:
                    continue
                share = np.zeros((Q, 16))
                for t0 in range(lo, hi, TILE):
                    for tx in range(16):
                        for n in range(4):
                            j = t0 + 4 * tx + n
                            if j < hi:
                                share[:, tx] = share[:, tx] + V[:, j]
                t = butterfly16(share)
                mine = q_label == c
                part_a[p] = np.where(mine, t, part_a[p])
                part_b[p] = np.where(mine, part_b[p], min_keep_nan(part_b[p], t / float(hi - lo)))
    return part_a, part_b


def finish_rows(part_a, part_b, q_label, seg, K, N):
    """(s, a, b) of sv_sil_finish: the states in the order of p, then the per-row rule"""
    with np.errstate(invalid="ignore", over="ignore"):
        ta, tb = part_a[0].copy(), part_b[0].copy()
        for p in range(1, part_a.shape[0]):
            ta = ta + part_a[p]
            tb = min_keep_nan(tb, part_b[p])
    return silhouette_of(ta, tb, q_label, seg, K, N)


def tree256(sh):
    """the binary tree sh[t] += sh[t + h], h = 128 .. 1 over [256, ...] shares"""
    h = 128
    with np.errstate(invalid="ignore", over="ignore"):
        while h:
            sh[:h] = sh[:h] + sh[h:2 * h]
            h >>= 1
    return sh[0]


def merge_order_sums(values, take):
    """sum of values[i] over the rows with take[i], in the merge order: thread t of 256 adds its rows t, t + 256, .. in order from 0.0,
    then the tree.  values: [n] or [n, m] (m sums side by side)"""
    values = np.asarray(values, dtype=np.float64)
    sh = np.zeros((256,) + values.shape[1:])
    with np.errstate(invalid="ignore", over="ignore"):
        for i0 in range(0, len(values), 256):
            chunk, tk = values[i0:i0 + 256], take[i0:i0 + 256]
            tk = tk.reshape((-1,) + (1,) * (values.ndim - 1))
            sh[:len(chunk)] = np.where(tk, sh[:len(chunk)] + chunk, sh[:len(chunk)])
    return tree256(sh)


def cluster_sums(s, q_label, K):
    """(cluster_sum float64 [K], cluster_cnt int64 [K], skipped) of sv_sil_finish's second launch"""
    s, q_label = np.asarray(s, dtype=np.float64), np.asarray(q_label, dtype=np.int64)
    good = ~np.isnan(s)
    sums = np.array([merge_order_sums(s, good & (q_label == c)) for c in range(K)])
    cnts = np.array([int((good & (q_label == c)).sum()) for c in range(K)], dtype=np.int64)
    return sums, cnts, int((~good).sum())


def spread(x, label, c, K):
    """(d2 fp32 [N], stat float64 [K, 2], cnt int64 [K]) of sv_cluster_spread"""
    label = np.asarray(label, dtype=np.int64)
    known = (label >= 0) & (label < K)
    full = pair_values32(RBF, x, c)
    d2 = np.where(known, full[np.arange(len(label)), np.where(known, label, 0)], np.float32(np.nan)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        both = np.stack([d2.astype(np.float64), np.sqrt(d2).astype(np.float64)], axis=1)
    stat = np.array([merge_order_sums(both, label == k) for k in range(K)]).reshape(K, 2)
    cnt = np.array([int((label == k).sum()) for k in range(K)], dtype=np.int64)
    return d2, stat, cnt


# ---------------------------------------------------------------------------------------------- Calinski-Harabasz, Davies-Bouldin
def centroids_of(x, labels, k):
    """(centroids float64 [k, d], counts int64 [k]): zeros for an empty cluster; what belongs to no cluster is left out"""
    x, labels = np.asarray(x, dtype=np.float64), np.asarray(labels, dtype=np.int64)
    ok = (labels >= 0) & (labels < k) & np.isfinite(x).all(axis=1)
    cent, cnt = np.zeros((k, x.shape[1])), np.zeros(k, dtype=np.int64)
    for c in range(k):
        rows = x[ok & (labels == c)]
        cnt[c] = len(rows)
        if len(rows):
            cent[c] = rows.mean(axis=0)
    return cent, cnt


def spread_of(x, labels, k, cent=None):
    """(centroids, counts, within float64 [k], mean_dist float64 [k]) in float64 with direct differences about `cent` (default: the
    float64 means)"""
    x, labels = np.asarray(x, dtype=np.float64), np.asarray(labels, dtype=np.int64)
    c64, cnt = centroids_of(x, labels, k)
    cent = c64 if cent is None else np.asarray(cent, dtype=np.float64)
    ok = (labels >= 0) & (labels < k) & np.isfinite(x).all(axis=1)
    within, mean_dist = np.zeros(k), np.zeros(k)
    for c in range(k):
        rows = x[ok & (labels == c)]
        if len(rows):
            d2 = ((rows - cent[c][None, :]) ** 2).sum(axis=1)
            within[c] = d2.sum()
            mean_dist[c] = np.sqrt(d2).mean()
    return cent, cnt, within, mean_dist


def calinski_harabasz(x, labels, k):
    cent, cnt, within, _ = spread_of(x, labels, k)
    keep = cnt > 0
    n, kk = int(cnt.sum()), int(keep.sum())
    x, labels = np.asarray(x, dtype=np.float64), np.asarray(labels, dtype=np.int64)
    ok = (labels >= 0) & (labels < k) & np.isfinite(x).all(axis=1)
    mean = x[ok].mean(axis=0)
    extra = float((cnt[keep] * ((cent[keep] - mean[None, :]) ** 2).sum(axis=1)).sum())
    intra = float(within.sum())
    return 1.0 if intra == 0.0 else extra * (n - kk) / (intra * (kk - 1.0))


def davies_bouldin(x, labels, k):
    cent, cnt, _, mean_dist = spread_of(x, labels, k)
    keep = cnt > 0
    c, s = cent[keep], mean_dist[keep]
    m = np.sqrt(((c[:, None, :] - c[None, :, :]) ** 2).sum(axis=2))
    if np.allclose(s, 0.0) or np.allclose(m, 0.0):
        return 0.0
    m[m == 0.0] = np.inf
    ratio = (s[:, None] + s[None, :]) / m
    np.fill_diagonal(ratio, 0.0)
    return float(ratio.max(axis=1).mean())


def indices_allowance(x, labels, k):
    """the 8x rule for the two centroid indices: 8 x the error of the fp32 restatement -- the float64 means rounded once to fp32, the
    kernel's fp32 squared distances to them and their fp32 roots, float64 sums, the host formulas -- against the float64 one.
    -> ((tol_ch, tol_db), (ch, db) in float64)"""
    from shot_vae_amd import validity as V
    x, labels = np.asarray(x, dtype=np.float64), np.asarray(labels, dtype=np.int64)
    cent, cnt = centroids_of(x, labels, k)
    c32 = cent.astype(np.float32).astype(np.float64)
    ok = (labels >= 0) & (labels < k) & np.isfinite(x).all(axis=1)
    d2, _, _ = spread(np.where(ok[:, None], x, 0.0), np.where(ok, labels, -1), c32, k)
    within = np.array([d2[ok & (labels == c)].astype(np.float64).sum() for c in range(k)])
    mean_dist = np.array([np.sqrt(d2[ok & (labels == c)]).astype(np.float64).mean() if cnt[c] else 0.0 for c in range(k)])
    ch, db = calinski_harabasz(x, labels, k), davies_bouldin(x, labels, k)
    ch32, db32 = V.calinski_harabasz(c32, cnt, within), V.davies_bouldin(c32, cnt, mean_dist)
    return (8.0 * abs(ch32 - ch), 8.0 * abs(db32 - db)), (ch, db)


# ---------------------------------------------------------------------------------------------- the tests' inputs
SHAPES_CPU = [(130, 3, 17), (449, 10, 128), (257, 65, 16), (65, 2, 1)]
SHAPES_GPU = [(2, 2, 1), (65, 2, 1), (63, 3, 15), (130, 10, 16), (193, 65, 17), (257, 10, 128), (449, 257, 33)]
BOUNDARY = (259, 5, 17, (64, 65, 129, 1, 0))                   # N, K, D and the exact cluster sizes
P_LIST = (1, 2, 3, 7, 64)
STREAM = 4500


def rows(n, D, stream):
    """fp32 values as float64: the posterior means of tests/_knn_ref.posterior"""
    from tests import _knn_ref as KR
    return KR.posterior(n, D, stream)[0]


def partition(N, K, seed, empty=True):
    """int64 [N] in shuffled order: cluster 0 is a singleton, cluster K - 1 is empty (K >= 3 and `empty`), the others share the rest with
    every one of them non-empty while rows last"""
    rs = np.random.RandomState(seed)
    last = K - 1 if (K >= 3 and empty) else K
    lab = np.empty(N, dtype=np.int64)
    lab[0] = 0
    if N > 1:
        pool = np.arange(1, last) if last > 1 else np.array([0])
        rest = N - 1
        lead = pool[:min(rest, len(pool))]
        lab[1:1 + len(lead)] = lead
        lab[1 + len(lead):] = pool[rs.randint(0, len(pool), rest - len(lead))]
    return lab[rs.permutation(N)]


def case(N, K, D, seed=0, empty=True):
    """(x float64 [N, D] of fp32 values, labels int64 [N]): clustered rows -- a per-cluster shift on top of the seeded rows -- with a
    singleton (cluster 0), an empty cluster (K - 1, for K >= 3) and duplicate rows: the first two rows of the largest cluster coincide"""
    lab = partition(N, K, STREAM + seed + 7 * N + K, empty)
    x = rows(N, D, STREAM + seed + N + D)
    shift = np.random.RandomState(STREAM + seed + K).randn(K, D)
    x = (x + 1.5 * shift[lab]).astype(np.float32).astype(np.float64)
    sizes = np.bincount(lab, minlength=K)
    big = int(np.argmax(sizes))
    members = np.nonzero(lab == big)[0]
    if len(members) >= 2:
        x[members[1]] = x[members[0]]
    return x, lab


def boundary_case():
    N, K, D, sizes = BOUNDARY
    lab = np.repeat(np.arange(K), sizes)
    lab = lab[np.random.RandomState(STREAM + 99).permutation(N)]
    x = rows(N, D, STREAM + 98)
    shift = np.random.RandomState(STREAM + 97).randn(K, D)
    return (x + 1.5 * shift[lab]).astype(np.float32).astype(np.float64), lab


def integer_case(D, N=130, K=4, seed=0):
    """integer data on which every distance, sum and hence a, b, s is exact: D = 1 with integer coordinates, or D = 17 with rows t_i x a
    fixed 0/1 pattern of four ones, so that every distance is 2 |t_i - t_j| (its square 4 (t_i - t_j)^2 is exact in fp32).
    -> (x, labels, t): t the integers"""
    rs = np.random.RandomState(STREAM + 50 + D + seed)
    lab = partition(N, K, STREAM + 51 + D + seed, empty=True)
    t = rs.randint(-40, 41, N) + 100 * lab
    if D == 1:
        return t[:, None].astype(np.float64), lab, t
    pattern = np.zeros(D)
    pattern[[0, 5, 15, 16]] = 1.0                               # both 16-blocks of D = 17
    return t[:, None] * pattern[None, :], lab, t


def integer_silhouette(t, scale, labels, K, metric=EUCLID):
    """(s, a, b) of an integer case in the caller's order from integer sums: distance scale |t_i - t_j| (its square under SQEUCLID)"""
    t, labels = np.asarray(t, dtype=np.int64), np.asarray(labels, dtype=np.int64)
    d = scale * np.abs(t[:, None] - t[None, :])
    if metric == SQEUCLID:
        d = d * d
    n = len(t)
    sizes = np.bincount(labels, minlength=K)
    ta, tb = np.zeros(n), np.full(n, np.inf)
    for c in range(K):
        if sizes[c] == 0:
            continue
        tot = d[:, labels == c].sum(axis=1).astype(np.float64)        # exact: far below 2^53
        mine = labels == c
        ta = np.where(mine, tot, ta)
        tb = np.where(mine, tb, np.minimum(tb, tot / float(sizes[c])))
    seg = np.concatenate([[0], np.cumsum(sizes)])
    return silhouette_of(ta, tb, labels, seg, K, n)
