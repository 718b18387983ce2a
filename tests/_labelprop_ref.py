"""Float64 numpy restatement of label spreading / propagation (shot_vae_amd.propagate, csrc/labelprop.hip), in two
forms: dense matrices in float64 (pinned to scikit-learn and to the closed form by tests/test_labelprop_cpu.py), and a walk over a
CSR graph in the kernels' own order -- fp32 storage, exact products, double additions in segment order, one rounding per operation --
which the GPU tests compare bit for bit."""
import numpy as np

SYM, ROW = 0, 1
SPREADING, PROPAGATION, PRODUCT = 0, 1, 2
EPS32 = float(np.finfo(np.float32).eps)


# ================================================================================================ inputs
def blobs(n, d, k, seed, scale=1.2):
    """k overlapping blobs of fp32 values: centres scale x normal, unit noise; row i belongs to class i mod k -> (rows, classes)"""
    rng = np.random.default_rng(seed)
    cen = scale * rng.standard_normal((k, d))
    y = np.arange(n) % k
    x = cen[y] + rng.standard_normal((n, d))
    return x.astype(np.float32).astype(np.float64), y.astype(np.int64)


def few_labels(y, k, per_class, seed):
    """-> y with all but `per_class` labels of every class replaced by -1"""
    rng = np.random.default_rng(seed)
    out = np.full_like(y, -1)
    for c in range(k):
        rows = np.nonzero(y == c)[0]
        keep = rng.permutation(rows)[:per_class]
        out[keep] = c
    return out


def knn_lists(x, k):
    """-> (dist [N, k], idx [N, k]): the k nearest other rows by squared Euclidean distance, closest first, ties by the smaller index"""
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d2, np.inf)
    idx = np.argsort(d2, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(d2, idx, axis=1), idx.astype(np.int64)


def dense_graph(idx, p=None, scaled=True):
    """embed.symmetrize restated densely: (A + A^T) / (2N) with A[i, idx[i, s]] = p[i, s] (1 without p); scaled=False leaves the
    1 / (2N) out.  Symmetric, zero diagonal."""
    n = idx.shape[0]
    a = np.zeros((n, n))
    p = np.ones(idx.shape) if p is None else p
    for i in range(n):
        for s in range(idx.shape[1]):
            if idx[i, s] >= 0 and p[i, s] > 0:
                a[i, idx[i, s]] = p[i, s]
    w = a + a.T
    return w / (2.0 * n) if scaled else w


def to_csr(w):
    """a dense matrix as CSR with ascending columns and fp32 values -> (rowptr, col, val)"""
    n = w.shape[0]
    rowptr, col, val = [0], [], []
    for i in range(n):
        nz = np.nonzero(w[i])[0]
        col.extend(nz.tolist())
        val.extend(w[i, nz].tolist())
        rowptr.append(len(col))
    return np.array(rowptr, dtype=np.int64), np.array(col, dtype=np.int64), np.array(val, dtype=np.float32)


def to_dense(rowptr, col, val, n, m=None):
    """the CSR entries that are edges as a dense float64 matrix [n, m]"""
    m = n if m is None else m
    w = np.zeros((n, m))
    for i in range(n):
        for q in range(rowptr[i], rowptr[i + 1]):
            if 0 <= col[q] < m:
                w[i, col[q]] += float(val[q])
    return w


def one_hot(y, k):
    f = np.zeros((len(y), k))
    ok = (y >= 0) & (y < k)
    f[np.nonzero(ok)[0], y[ok]] = 1.0
    return f


# ================================================================================================ the dense form, float64
def normalize(w, mode):
    """SYM: D^-1/2 W D^-1/2; ROW: D^-1 W; a degree of 0 gives zeros"""
    deg = w.sum(axis=1)
    if mode == SYM:
        dd = np.outer(deg, deg)
        return np.where(dd == 0.0, 0.0, w / np.sqrt(np.where(dd == 0.0, 1.0, dd)))
    return np.where(deg[:, None] == 0.0, 0.0, w / np.where(deg == 0.0, 1.0, deg)[:, None])


def step(s, f, y, variant, alpha=0.2, dtype=np.float64):
    """one iteration on a dense iteration matrix; dtype=np.float32 is the fp32 restatement the allowances are measured with"""
    k = f.shape[1]
    s, f = s.astype(dtype), f.astype(dtype)
    acc = s @ f
    if variant == PRODUCT:
        return acc
    hot = one_hot(y, k).astype(dtype)
    if variant == SPREADING:
        return dtype(alpha) * acc + dtype(1.0 - alpha) * hot
    norm = acc.sum(axis=1, keepdims=True)
    norm[norm == 0] = 1
    labelled = ((y >= 0) & (y < k))[:, None]
    return np.where(labelled, hot, acc / norm)


def iterate(s, y, k, variant, alpha=0.2, max_iter=30, tol=1e-3, check_every=1, dtype=np.float64):
    """scikit-learn's loop from the one-hot labels: the run ends at the first iteration t < max_iter that is a multiple of check_every
    and has sum |F_t - F_t-1| < tol, else at max_iter -> (F, n_iter, converged, the deltas of all iterations)"""
    f = one_hot(y, k).astype(dtype)
    deltas = []
    for it in range(1, max_iter + 1):
        new = step(s, f, y, variant, alpha, dtype)
        deltas.append(float(np.abs(new.astype(np.float64) - f.astype(np.float64)).sum()))
        f = new
        if it % check_every == 0 and it < max_iter and deltas[-1] < tol:
            return f, it, True, deltas
    return f, max_iter, False, deltas


def finish(f):
    """-> (proba, pred, conf, (decided, unreached)): the rows over their sums (0 -> 1), the first maximum, -1 on a row whose sum is 0
    or that holds a NaN"""
    f = np.asarray(f, dtype=np.float64)
    s = f.sum(axis=1)
    nan = np.isnan(f).any(axis=1)
    proba = f / np.where(s == 0.0, 1.0, s)[:, None]
    best = np.where(nan, 0, np.argmax(np.where(np.isnan(f), -np.inf, f), axis=1))
    pred = np.where(nan | (s == 0.0), -1, best)
    conf = proba[np.arange(len(f)), best]
    return proba, pred.astype(np.int64), conf, (int((~nan & (s != 0.0)).sum()), int((~nan & (s == 0.0)).sum()))


def closed_form(s, y, k, alpha):
    """the fixed point of spreading: (1 - alpha) (I - alpha S)^-1 Y"""
    return (1.0 - alpha) * np.linalg.solve(np.eye(s.shape[0]) - alpha * s, one_hot(y, k))


def margin(f):
    """the gap between the largest and the second largest entry of every row (inf for one class)"""
    if f.shape[1] < 2:
        return np.full(f.shape[0], np.inf)
    top = np.sort(f, axis=1)
    return top[:, -1] - top[:, -2]


def half_ulp32(a):
    return 0.5 * EPS32 * float(np.max(np.abs(a))) if np.size(a) else 0.0


def allowance(f32, f64):
    """the project's 8x rule: 8 x the error of the fp32 restatement against float64, never less than 8 half ulps of fp32 at the
    largest value"""
    return 8.0 * max(float(np.max(np.abs(np.asarray(f32, dtype=np.float64) - f64))), half_ulp32(f64))


# ================================================================================================ the CSR form, in the kernels' order
def _segment(rowptr, i, nnz):
    return min(max(int(rowptr[i]), 0), nnz), min(max(int(rowptr[i + 1]), 0), nnz)


def csr_degrees(rowptr, col, val, n):
    """sv_lp_normalize's deg: lane s of eight adds the valid entries s, s + 8, .. in order; the lane sums meet as
    ((l0 + l4) + (l2 + l6)) + ((l1 + l5) + (l3 + l7))"""
    nnz = len(col)
    deg = np.zeros(n)
    for i in range(n):
        beg, end = _segment(rowptr, i, nnz)
        lane = [0.0] * 8
        for s in range(8):
            for q in range(beg + s, end, 8):
                if 0 <= col[q] < n:
                    lane[s] = lane[s] + float(val[q])
        deg[i] = ((lane[0] + lane[4]) + (lane[2] + lane[6])) + ((lane[1] + lane[5]) + (lane[3] + lane[7]))
    return deg


def csr_normalize(rowptr, col, val, n, mode, deg=None):
    """sv_lp_normalize's sval: product, root and quotient rounded once each in double, the result once to fp32"""
    nnz = len(col)
    deg = csr_degrees(rowptr, col, val, n) if deg is None else deg
    sval = np.zeros(nnz, dtype=np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(n):
            beg, end = _segment(rowptr, i, nnz)
            for q in range(beg, end):
                j = col[q]
                if not 0 <= j < n:
                    continue
                w = np.float64(val[q])
                if mode == SYM:
                    dd = np.float64(deg[i]) * np.float64(deg[j])
                    sval[q] = np.float32(0) if dd == 0.0 else np.float32(w / np.sqrt(dd))
                else:
                    sval[q] = np.float32(0) if deg[i] == 0.0 else np.float32(w / np.float64(deg[i]))
    return sval, deg


def csr_step(rowptr, col, sval, f_in, n, k, label, variant, alpha=0.2, one_minus_alpha=None):
    """sv_lp_step bit for bit: f_in fp32 [m, k] -> fp32 [n, k].  acc adds the exact products of a row's valid entries in segment order
    from 0.0 (cumsum is sequential); the propagation variant's row sum runs in CLASS ORDER from 0.0."""
    f_in = np.asarray(f_in, dtype=np.float32)
    m, nnz = f_in.shape[0], len(col)
    oma = (1.0 - alpha) if one_minus_alpha is None else one_minus_alpha
    out = np.zeros((n, k), dtype=np.float32)
    f64 = f_in.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            beg, end = _segment(rowptr, i, nnz)
            qs = [q for q in range(beg, end) if 0 <= col[q] < m]
            lab = int(label[i]) if label is not None else -1
            labelled = 0 <= lab < k
            if qs:
                prod = sval[qs].astype(np.float64)[:, None] * f64[col[qs]]
                acc = np.cumsum(np.concatenate([np.zeros((1, k)), prod]), axis=0)[-1]
            else:
                acc = np.zeros(k)
            if variant == SPREADING:
                add = np.zeros(k)
                if labelled:
                    add[lab] = oma
                out[i] = (np.float64(alpha) * acc + add).astype(np.float32)
            elif variant == PROPAGATION:
                if labelled:
                    out[i] = 0
                    out[i, lab] = 1
                else:
                    s = np.cumsum(np.concatenate([[0.0], acc]))[-1]
                    out[i] = (acc / (1.0 if s == 0.0 else s)).astype(np.float32)
            else:
                out[i] = acc.astype(np.float32)
    return out


def csr_iterate(rowptr, col, sval, y, n, k, variant, alpha=0.2, max_iter=30, tol=1e-3, check_every=1):
    """the device's fit, emulated: csr_step from the one-hot labels with fp32 storage, the deltas in float64
    -> (F fp32, n_iter, converged, deltas)"""
    f = one_hot(y, k).astype(np.float32)
    deltas = []
    for it in range(1, max_iter + 1):
        new = csr_step(rowptr, col, sval, f, n, k, y, variant, alpha)
        deltas.append(float(np.abs(new.astype(np.float64) - f.astype(np.float64)).sum()))
        f = new
        if it % check_every == 0 and it < max_iter and deltas[-1] < tol:
            return f, it, True, deltas
    return f, max_iter, False, deltas


def csr_finish(f):
    """sv_lp_finish: the sum in class order in double, the quotient rounded once -> (proba fp32, pred, conf fp32, counts)"""
    f = np.asarray(f, dtype=np.float32)
    n, k = f.shape
    s = np.cumsum(np.concatenate([np.zeros((n, 1)), f.astype(np.float64)], axis=1), axis=1)[:, -1]
    nan = np.isnan(f).any(axis=1)
    div = np.where(s == 0.0, 1.0, s)
    with np.errstate(invalid="ignore"):
        proba = (f.astype(np.float64) / div[:, None]).astype(np.float32)
        best = np.zeros(n, dtype=np.int64)
        for i in range(n):
            top = f[i, 0]
            for c in range(k):
                if f[i, c] > top:
                    top, best[i] = f[i, c], c
    pred = np.where(nan | (s == 0.0), -1, best).astype(np.int64)
    conf = proba[np.arange(n), best]
    return proba, pred, conf, (int((~nan & (s != 0.0)).sum()), int((~nan & (s == 0.0)).sum()))
