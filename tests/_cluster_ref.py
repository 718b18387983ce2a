"""numpy float64 restatement of csrc/cluster.hip's and shot_vae_amd/cluster.py's definitions (include/shotvae_hip.h):
the assignment with the first-minimum and -1 rules, a Lloyd iteration that keeps the centroid of an empty cluster, D^2 seeding from
given uniforms, the contingency table, every partition metric from its textbook formula, and a brute-force best matching over
permutations.  tests/test_cluster_cpu.py pins the metrics to scikit-learn and scipy; the GPU tests measure their allowances with it."""
import itertools
import math

import numpy as np


def distances(x, c, dtype=np.float64):
    """[n, k] squared Euclid distances in `dtype`, sums over the differences themselves"""
    x, c = np.asarray(x, dtype=dtype), np.asarray(c, dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        d = x[:, None, :] - c[None, :, :]
        return np.sum(d * d, axis=2)


def assign(x, c, dist=None):
    """(assign int64 [n], dist float64 [n]): the smallest index of the minimum over the finite distances; -1 / +inf when none is finite"""
    d = distances(x, c) if dist is None else np.asarray(dist, dtype=np.float64)
    key = np.where(np.isfinite(d), d, np.inf)
    a = np.argmin(key, axis=1).astype(np.int64)           # (the first minimum)
    v = key[np.arange(len(key)), a]
    a[~np.isfinite(v)] = -1
    return a, v


def margin(x, c):
    """the float64 gap between the best and the second-best centroid of every row (+inf with one centroid)"""
    d = np.sort(distances(x, c), axis=1)
    return d[:, 1] - d[:, 0] if d.shape[1] > 1 else np.full(len(d), np.inf)


def allowance(x, c):
    """the 8x rule of tests/test_knn_gpu.py for the Euclid value on these inputs: 8 x the largest error of the fp32 restatement
    against float64"""
    ref = distances(x, c)
    f32 = distances(x, c, dtype=np.float32).astype(np.float64)
    fin = np.isfinite(ref) & np.isfinite(f32)
    return 8.0 * float(np.max(np.abs(f32 - ref)[fin], initial=0.0))


def update(x, a, c_old, dist=None):
    """(c_new float64 [k, d], count int64 [k], sums float64 [k, d], inertia) of the assignment a: the mean of every cluster's rows, the OLD centroid
    for an empty cluster; rows with a outside [0, k) are skipped"""
    x, c_old = np.asarray(x, dtype=np.float64), np.asarray(c_old, dtype=np.float64)
    k = c_old.shape[0]
    ok = (a >= 0) & (a < k)
    sums = np.zeros_like(c_old)
    np.add.at(sums, a[ok], x[ok])
    count = np.bincount(a[ok], minlength=k).astype(np.int64)
    c_new = np.where(count[:, None] > 0, sums / np.maximum(count, 1)[:, None], c_old)
    inertia = float(np.sum(np.asarray(dist, dtype=np.float64)[ok])) if dist is not None else 0.0
    return c_new, count, sums, inertia


def shift(c_new, c_old):
    return float(np.sum((np.asarray(c_new, dtype=np.float64) - np.asarray(c_old, dtype=np.float64)) ** 2))


def lloyd(x, c):
    """one iteration: (assign, c_new, count, inertia about c)"""
    a, v = assign(x, c)
    c_new, count, _, inertia = update(x, a, c, v)
    return a, c_new, count, inertia


def plus_plus(x, k, u):
    """the row indices of D^2 seeding from the uniforms u [k]: floor(u[0] n), then the first row whose running sum of min-distances
    exceeds u[j] x the total"""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    idx = [min(max(int(math.floor(u[0] * n)), 0), n - 1)]
    mind = np.full(n, np.inf)
    for j in range(1, k):
        mind = np.minimum(mind, distances(x, x[idx[-1]:idx[-1] + 1])[:, 0])
        cum = np.cumsum(mind)
        idx.append(min(int(np.searchsorted(cum, u[j] * cum[-1], side="right")), n - 1))
    return np.array(idx, dtype=np.int64)


def contingency(a, b, ka, kb):
    a, b = np.asarray(a), np.asarray(b)
    ok = (a >= 0) & (a < ka) & (b >= 0) & (b < kb)
    t = np.zeros((ka, kb), dtype=np.int64)
    np.add.at(t, (a[ok], b[ok]), 1)
    return t, np.array([int(ok.sum()), len(a)], dtype=np.int64)


def best_matching(table):
    """the largest sum of a one-to-one matching of rows to columns, by trying every injection of the smaller side (K <= 6 or so)"""
    t = np.asarray(table)
    if t.shape[0] > t.shape[1]:
        t = t.T
    n, m = t.shape
    return max(sum(t[i, p[i]] for i in range(n)) for p in itertools.permutations(range(m), n))


def best_matching_dp(table):
    """the same maximum by dynamic programming over subsets of the smaller side (exact, up to 16 or so on that side): the tables
    too large for the permutations; tests/test_cluster_cpu.py holds it to best_matching"""
    t = np.asarray(table)
    if t.shape[0] < t.shape[1]:
        t = t.T
    n, m = t.shape                                       # m <= n: every column of t is matched to a distinct row
    best = {0: 0}
    for i in range(n):
        nxt = dict(best)                                  # row i stays unmatched
        for mask, v in best.items():
            for j in range(m):
                if not mask >> j & 1:
                    w = v + int(t[i, j])
                    if nxt.get(mask | 1 << j, -1) < w:
                        nxt[mask | 1 << j] = w
        best = nxt
    return best[(1 << m) - 1]


def _h(counts):
    p = np.asarray(counts, dtype=np.float64)
    p = p[p > 0] / p.sum()
    return float(-(p * np.log(p)).sum())


def metrics(table):
    """every metric of partition_metrics from its definition (rows: classes, columns: clusters)"""
    t = np.asarray(table, dtype=np.float64)
    n = t.sum()
    a, b = t.sum(axis=1), t.sum(axis=0)
    ha, hb = _h(a), _h(b)
    mi = 0.0
    for i in range(t.shape[0]):
        for j in range(t.shape[1]):
            if t[i, j] > 0:
                mi += t[i, j] / n * math.log(t[i, j] * n / (a[i] * b[j]))
    mi = max(mi, 0.0)
    c2 = lambda v: float(sum(math.comb(int(c), 2) for c in np.ravel(v)))          # noqa: E731
    index, ea, eb, total = c2(t), c2(a), c2(b), math.comb(int(n), 2)
    if ea == index and eb == index:
        ari = 1.0                                           # identical partitions (a single row included)
    else:
        expected = ea * eb / total
        ari = (index - expected) / (0.5 * (ea + eb) - expected)
    hom = 1.0 if ha == 0.0 else mi / ha
    com = 1.0 if hb == 0.0 else mi / hb
    return dict(accuracy=(best_matching(table) if max(t.shape) <= 7 else best_matching_dp(table)) / n, purity=float(t.max(axis=0).sum() / n),
                nmi=1.0 if ha == 0.0 and hb == 0.0 else mi / (0.5 * (ha + hb)), ari=ari, homogeneity=hom, completeness=com,
                v_measure=0.0 if hom + com == 0.0 else 2.0 * hom * com / (hom + com), n=int(n))


def blobs(n, k, d, stream, spread=0.25, scale=4.0):
    """n rows around k separated centres (fp32 values as float64): centre j on an integer lattice point of side `scale`, the noise
    uniform in [-spread, spread) -- closed forms of oracle/closed_form.py, so the rows are the same everywhere.
    -> (rows [n, d], centres [k, d], the blob of every row)"""
    from oracle import closed_form as CF
    cen = np.floor(CF.uniform((k, d), stream, -3.0, 4.0).numpy().astype(np.float64)) * scale
    # distinct centres: add the index along the first dimension (a different lattice point per blob)
    cen[:, 0] += 8.0 * scale * np.arange(k)
    which = (np.arange(n) * 7 + 3) % k
    noise = CF.uniform((n, d), stream + 1, -spread, spread).numpy().astype(np.float64)
    rows = (cen[which] + noise).astype(np.float32).astype(np.float64)
    return rows, cen, which
