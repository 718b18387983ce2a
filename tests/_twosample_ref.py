"""numpy restatement of csrc/ksum.hip's definitions (include/shotvae_hip.h: sv_ksum_scan, sv_ksum_finish) and of
shot_vae_amd/twosample.py, in two forms: a DENSE one in float64 (the kernel matrix, numpy's own sums) and one that walks tiles, columns
and partial states IN THE KERNEL'S ORDER with the kernel's fp32 pair values (exact emulation of fmaf: round to odd in double, then once
to fp32).  tests/test_twosample_cpu.py pins the dense form to scikit-learn and to hand-written sums; the GPU tests compare the kernels
with both and take their allowances from here, never from a GPU result."""
import numpy as np

RBF, IMQ, POLY = 0, 1, 2
KIND = {"rbf": RBF, "imq": IMQ, "poly": POLY}
U53 = 2.0 ** -53
TILE = 64


# ---------------------------------------------------------------------------------------------- pair values
def pair_values(kind, q, g):
    """float64 [Q, N]: |q_i - g_j|^2 from the differences themselves (RBF, IMQ) or q_i . g_j (POLY)"""
    q, g = np.asarray(q, dtype=np.float64), np.asarray(g, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if kind == POLY:
            return q @ g.T
        d = q[:, None, :] - g[None, :, :]
        return np.sum(d * d, axis=2)


def fmaf32(a, b, c):
    """the fp32 fused multiply-add, exactly: the product of two fp32 values is exact in double; the sum with c is rounded TO ODD in
    double (TwoSum gives the error's sign), which makes the second rounding to fp32 the correct one"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        t = s - p
        e = (p - (s - t)) + (c - t)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0.0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(e > 0.0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def pair_values32(kind, q, g):
    """fp32 [Q, N] by the kernel's rule: 16 dimensions in fp32 with fmaf in index order from 0, the 16-blocks added in double in index
    order, rounded once to fp32 -- sv_pairdist's SV_DIST_EUCLID value bit for bit (POLY: fmaf(q, g, part) in place of the difference)"""
    q, g = np.asarray(q, dtype=np.float32), np.asarray(g, dtype=np.float32)
    Q, N, D = q.shape[0], g.shape[0], q.shape[1]
    acc = np.zeros((Q, N), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for d0 in range(0, D, 16):
            part = np.zeros((Q, N), dtype=np.float32)
            for d in range(d0, min(d0 + 16, D)):
                a = np.broadcast_to(q[:, d][:, None], (Q, N))
                b = np.broadcast_to(g[:, d][None, :], (Q, N))
                if kind == POLY:
                    part = fmaf32(a, b, part)
                else:
                    dm = (a - b).astype(np.float32)
                    part = fmaf32(dm, dm, part)
            acc = acc + part.astype(np.float64)
        return acc.astype(np.float32)


# ---------------------------------------------------------------------------------------------- kernel functions
def params(kind, gammas, coef0=1.0, weights=None):
    """the parameter array double [n_scale, 2]: (a_s, w_s) with equal weights 1 / n_scale, or (gamma, coef0) for POLY"""
    a = np.atleast_1d(np.asarray(gammas, dtype=np.float64))
    if kind == POLY:
        return np.array([[a[0], float(coef0)]])
    w = np.full(len(a), 1.0 / len(a)) if weights is None else np.asarray(weights, dtype=np.float64)
    return np.stack([a, w], axis=1)


def kernel_value(kind, x, kparam, degree=3):
    """k from the pair value x (any shape, taken to float64) with the kernel's operations in the kernel's order, each rounded once"""
    x = np.asarray(x).astype(np.float64)
    kparam = np.asarray(kparam, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if kind == POLY:
            b = kparam[0, 0] * x + kparam[0, 1]
            r = b
            for _ in range(1, degree):
                r = r * b
            return r
        k = np.zeros_like(x)
        for a, w in kparam:
            t = a * x
            k = k + (w * np.exp(-t) if kind == RBF else w / (1.0 + t))
        return k


def counted(Q, N, col0=0, self0=-1):
    """bool [Q, N]: the pair counts -- the self pair col0 + j == self0 + i does not"""
    m = np.ones((Q, N), dtype=bool)
    if self0 >= 0:
        i = np.arange(Q)[:, None]
        j = np.arange(N)[None, :]
        m &= (col0 + j) != (self0 + i)
    return m


def kernel_matrix(kind, kparam, degree, q, g, fp32=False):
    """float64 [Q, N]: the kernel function (float64) of the float64 pair values, or of the kernel's fp32 pair values"""
    v = pair_values32(kind, q, g) if fp32 else pair_values(kind, q, g)
    return kernel_value(kind, v, kparam, degree)


def dense_sums(kind, kparam, degree, q, g, w=None, col0=0, self0=-1, fp32=False, K=None):
    """float64 [Q]: sum_j w_j k(q_i, g_j) over the pairs that count, numpy's own summation.  A pair that does not count is left out by
    a mask, never by a product"""
    K = kernel_matrix(kind, kparam, degree, q, g, fp32) if K is None else K
    wv = np.ones(K.shape[1]) if w is None else np.asarray(w, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        terms = np.where(counted(K.shape[0], K.shape[1], col0, self0), wv[None, :] * K, 0.0)
    return terms.sum(axis=1)


def allowance(kind, kparam, degree, q, g, w=None, col0=0, self0=-1):
    """the 8x rule for the row sums of one case, one number: 8 x the largest error of the fp32 restatement (the kernel's fp32 pair
    values, float64 kernel function and sums) against the float64 one.  -> (allowance, the fp32 restatement's error)"""
    ref = dense_sums(kind, kparam, degree, q, g, w, col0, self0)
    f32 = dense_sums(kind, kparam, degree, q, g, w, col0, self0, fp32=True)
    fin = np.isfinite(ref) & np.isfinite(f32)
    err = float(np.max(np.abs(f32 - ref)[fin])) if fin.any() else 0.0
    return 8.0 * err, err


def effective_terms(kind, kparam, degree, q, g, w=None, col0=0, self0=-1):
    """float64 [Q]: (sum_j t_j)^2 / sum_j t_j^2 of the terms t_j = w_j k(q_i, g_j) that count"""
    K = kernel_matrix(kind, kparam, degree, q, g)
    wv = np.ones(K.shape[1]) if w is None else np.asarray(w, dtype=np.float64)
    t = np.where(counted(K.shape[0], K.shape[1], col0, self0), wv[None, :] * K, 0.0)
    return t.sum(axis=1) ** 2 / (t * t).sum(axis=1)


# ---------------------------------------------------------------------------------------------- the kernel's order
def butterfly16(share):
    """[rows, 16] -> [rows]: the 16 shares of a row as kn_aux_reduce adds them (x += shfl_xor(x, 8), 4, 2, 1: lane 0's value)"""
    a = share[:, :8] + share[:, 8:]
    b = a[:, :4] + a[:, 4:]
    c = b[:, :2] + b[:, 2:]
    return c[:, 0] + c[:, 1]


def ordered_parts(kind, kparam, degree, q, g, w=None, col0=0, self0=-1, P=1, K=None):
    """part float64 [P, Q] as sv_ksum_scan leaves it: state p takes the gallery tiles p, p + P, ..; thread tx of a row's 16 adds the
    columns 4 tx .. 4 tx + 3 of every tile in order, the products (double) w_j * k rounded once, from 0.0; the shares meet in the
    butterfly.  K: the kernel values [Q, N] to add (default: the float64 kernel function of the kernel's fp32 pair values)"""
    K = kernel_matrix(kind, kparam, degree, q, g, fp32=True) if K is None else np.asarray(K, dtype=np.float64)
    Q, N = K.shape
    wv = np.ones(N) if w is None else np.asarray(w, dtype=np.float32).astype(np.float64)
    ok = counted(Q, N, col0, self0)
    part = np.zeros((P, Q))
    with np.errstate(invalid="ignore", over="ignore"):
        for p in range(P):
            share = np.zeros((Q, 16))
            for g0 in range(p * TILE, N, P * TILE):
                for tx in range(16):
                    for n in range(4):
                        j = g0 + 4 * tx + n
                        if j < N:
                            term = wv[j] * K[:, j]
                            share[:, tx] = np.where(ok[:, j], share[:, tx] + term, share[:, tx])
            part[p] = butterfly16(share)
    return part


def finish_rows(part, into=None):
    """row_sum [Q] of part [P, Q]: the states in the order of p, then (accumulate) added to `into`"""
    with np.errstate(invalid="ignore", over="ignore"):
        t = part[0].copy()
        for p in range(1, part.shape[0]):
            t = t + part[p]
        return t if into is None else into + t


def finish_total(row_sum, q_w=None):
    """total of row_sum [Q]: thread t of 256 adds the rows t, t + 256, .. in order from 0.0 -- each the product (double) q_w[i] *
    row_sum[i], rounded once --, then the binary tree sh[t] += sh[t + h], h = 128 .. 1"""
    row_sum = np.asarray(row_sum, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        terms = row_sum if q_w is None else np.asarray(q_w, dtype=np.float32).astype(np.float64) * row_sum
        sh = np.zeros(256)
        for i0 in range(0, len(terms), 256):
            chunk = terms[i0:i0 + 256]
            sh[:len(chunk)] = sh[:len(chunk)] + chunk
        h = 128
        while h:
            sh[:h] = sh[:h] + sh[h:2 * h]
            h >>= 1
        return sh[0]


# ---------------------------------------------------------------------------------------------- the statistics
def mmd2(kind, kparam, degree, x, y, unbiased=True, fp32=False):
    """the squared MMD in float64: the U-statistic without the self pairs, or the V-statistic with the diagonal"""
    n, m = len(x), len(y)
    self0 = 0 if unbiased else -1
    sxx = dense_sums(kind, kparam, degree, x, x, self0=self0, fp32=fp32).sum()
    syy = dense_sums(kind, kparam, degree, y, y, self0=self0, fp32=fp32).sum()
    sxy = dense_sums(kind, kparam, degree, x, y, fp32=fp32).sum()
    if unbiased:
        return sxx / (n * (n - 1)) + syy / (m * (m - 1)) - 2.0 * sxy / (n * m)
    return sxx / (n * n) + syy / (m * m) - 2.0 * sxy / (n * m)


def mmd2_allowance(kind, kparam, degree, x, y, unbiased=True):
    """propagated from the three sums, not relative to the small difference: each scan's row allowance (allowance()) times its rows,
    divided by the count its total is divided by, the cross term twice"""
    n, m = len(x), len(y)
    self0 = 0 if unbiased else -1
    axx = allowance(kind, kparam, degree, x, x, self0=self0)[0] * n / (n * (n - 1) if unbiased else n * n)
    ayy = allowance(kind, kparam, degree, y, y, self0=self0)[0] * m / (m * (m - 1) if unbiased else m * m)
    axy = allowance(kind, kparam, degree, x, y)[0] * n / (n * m)
    return axx + ayy + 2.0 * axy


def witness(kind, kparam, degree, x, y, at, fp32=False):
    return dense_sums(kind, kparam, degree, at, x, fp32=fp32) / len(x) - dense_sums(kind, kparam, degree, at, y, fp32=fp32) / len(y)


def kid(real, fake, ia, ib, degree=3, gamma=None, coef0=1.0):
    """(mean, population standard deviation, the values) of the unbiased polynomial MMD^2 over the subsets real[ia[s]], fake[ib[s]]"""
    real, fake = np.asarray(real, dtype=np.float64), np.asarray(fake, dtype=np.float64)
    kp = params(POLY, 1.0 / real.shape[1] if gamma is None else gamma, coef0)
    vals = np.array([mmd2(POLY, kp, degree, real[a], fake[b], True) for a, b in zip(ia, ib)])
    return float(vals.mean()), float(vals.std()), vals


def kid_allowance(real, fake, ia, ib, degree=3, gamma=None, coef0=1.0):
    """the largest mmd2_allowance over the subsets: it bounds the error of every value, hence of their mean and of their standard
    deviation (|std(a) - std(b)| <= max |a - b| ... x 2 for the centring)"""
    real, fake = np.asarray(real, dtype=np.float64), np.asarray(fake, dtype=np.float64)
    kp = params(POLY, 1.0 / real.shape[1] if gamma is None else gamma, coef0)
    return max(mmd2_allowance(POLY, kp, degree, real[a], fake[b], True) for a, b in zip(ia, ib))


def split_weights(member, n, m):
    """+m for a row of the first group, -n for the others (the weights +1 / n, -1 / m times n m)"""
    return np.where(np.asarray(member, dtype=bool), float(m), -float(n))


def permutation_stats(kind, kparam, degree, x, y, signs, fp32=False):
    """float64 [1 + B]: the V-statistic w^T K w / (n m)^2 of the identity split, then of each split of `signs` (bool [B, n + m])"""
    n, m = len(x), len(y)
    z = np.concatenate([np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)])
    K = kernel_matrix(kind, kparam, degree, z, z, fp32)
    member = np.concatenate([(np.arange(n + m) < n)[None, :], np.asarray(signs, dtype=bool)])
    W = split_weights(member, n, m)
    return np.einsum("bi,ij,bj->b", W, K, W) / (float(n) * float(m)) ** 2


def permutation_allowance(kind, kparam, degree, x, y):
    """8 x the fp32 restatement's error bound of one statistic, for every split at once: |w^T (K32 - K64) w| <= sum_ij |w_i w_j|
    |K32 - K64|_ij with |w| = 1 / n or 1 / m, plus the double roundings of (n + m)^2 terms of size |w_i w_j K_ij|"""
    n, m = len(x), len(y)
    z = np.concatenate([np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)])
    K64, K32 = kernel_matrix(kind, kparam, degree, z, z), kernel_matrix(kind, kparam, degree, z, z, True)
    a = np.where(np.arange(n + m) < n, 1.0 / n, 1.0 / m)
    A = np.outer(a, a)
    return 8.0 * float((A * np.abs(K32 - K64)).sum()) + (n + m + 8) * 2.0 * U53 * float((A * np.abs(K64)).sum())


def p_value(stats):
    return (1 + int(np.sum(stats[1:] >= stats[0]))) / len(stats)


def lower_median(values):
    """the lower median: the element of rank ceil(n / 2) (1-based) -- torch.kthvalue(.., (n + 1) // 2)"""
    v = np.sort(np.asarray(values).reshape(-1))
    return v[(len(v) + 1) // 2 - 1]


def median_bandwidth(rows):
    """1 / the lower median of the off-diagonal squared distances of `rows`, float64"""
    d = pair_values(RBF, rows, rows)
    off = d[~np.eye(len(d), dtype=bool)]
    return 1.0 / lower_median(off)


def rbf_prior_expectations(x, kparam):
    """E_y k(x_i, y) [n] and E k(y, y') for y, y' ~ N(0, I) under k = sum_s w_s exp(-a_s |.|^2)"""
    x = np.asarray(x, dtype=np.float64)
    D = x.shape[1]
    r2 = (x * x).sum(axis=1)
    exy, eyy = np.zeros(len(x)), 0.0
    for a, w in np.asarray(kparam, dtype=np.float64):
        exy += w * (1.0 + 2.0 * a) ** (-0.5 * D) * np.exp(-a * r2 / (1.0 + 2.0 * a))
        eyy += w * (1.0 + 4.0 * a) ** (-0.5 * D)
    return exy, eyy


# ---------------------------------------------------------------------------------------------- the GPU tests' inputs
SQ, SG = 4300, 4302                                             # the streams of the query and the gallery rows
SHAPES = [(1, 1, 1), (5, 2, 7), (70, 63, 17), (33, 65, 128), (70, 130, 130), (70, 130, 1)]
LADDER = (0.25, 0.5, 1.0, 2.0, 4.0)
# (kind, n_scale, degree) of the value cases: all three kinds, n_scale 1 and 5, degree 1 and 3
KERNELS = [("rbf", 1, 0), ("rbf", 5, 0), ("imq", 1, 0), ("imq", 5, 0), ("poly", 1, 1), ("poly", 1, 3)]
PERM_N, PERM_M, PERM_D, PERM_B, PERM_SEED = 40, 30, 17, 99, 4310


def rows(n, D, stream):
    """fp32 values as float64: the posterior means of tests/_knn_ref.posterior"""
    from tests import _knn_ref as R
    return R.posterior(n, D, stream)[0]


def case_rows(Q, N, D):
    return rows(Q, D, SQ), rows(N, D, SG)


def case_params(name, n_scale, degree, q, g):
    """the parameters of a value case: the median bandwidth of the pooled rows (1 where two rows coincide or there is one pair only)
    times LADDER's entries for five scales; POLY: gamma = 1 / D, coef0 = 1"""
    kind = KIND[name]
    if kind == POLY:
        return params(POLY, 1.0 / q.shape[1], 1.0)
    pooled = np.concatenate([q, g])
    a = median_bandwidth(pooled) if len(pooled) > 1 else 1.0
    if not np.isfinite(a):
        a = 1.0
    return params(kind, a * np.asarray(LADDER) if n_scale == 5 else [a])


def permutation_case():
    """(x, y, signs): two draws of one distribution and PERM_B seeded splits"""
    x, y = rows(PERM_N, PERM_D, SQ + 20), rows(PERM_M, PERM_D, SG + 20)
    rs = np.random.RandomState(PERM_SEED)
    signs = np.zeros((PERM_B, PERM_N + PERM_M), dtype=bool)
    for b in range(PERM_B):
        signs[b, rs.permutation(PERM_N + PERM_M)[:PERM_N]] = True
    return x, y, signs
