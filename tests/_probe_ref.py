"""Linear probes restated in numpy from the header comments of include/shotvae_hip.h (sv_probe_*): the score of a pair, the row pass, the
residuals and the gradient, the partial states in the kernel's own order, the Nesterov step and the whole fit, each in float64 (the
reference) or with float32 scores (the kernels' own precision, for the 8x rule).  numpy only: shared by tests/test_probe_cpu.py (which
pins it to torch.autograd and scikit-learn) and tests/test_probe_gpu.py."""
import math

import numpy as np

from tests._gmm_ref import blobs, half_ulp32          # noqa: F401  (inputs and the 8x rule's floor, shared with the mixtures)


# ------------------------------------------------------------------------------------------------ the row pass
def scores(x, w, b, dtype=np.float64):
    """v [N, K] = b_k + sum_d x_id w_kd; NaN for a row that is not finite"""
    x, w, b = np.asarray(x, dtype=dtype), np.asarray(w, dtype=dtype), np.asarray(b, dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (x @ w.T + b[None, :]).astype(dtype)
    v[~np.isfinite(x).all(axis=1)] = np.nan
    return v


def rows(x, w, b, y=None, dtype=np.float64):
    """-> (lse [N], loss [N] or None, pred int64 [N], proba [N, K]) of sv_probe_rows"""
    v = scores(x, w, b, dtype)
    K = v.shape[1]
    bad = np.isnan(v).any(axis=1)
    with np.errstate(invalid="ignore"):
        m = np.where(bad, 0.0, v.max(axis=1)).astype(dtype)
        lse = (m + np.log(np.exp(v - m[:, None]).sum(axis=1, dtype=dtype))).astype(dtype)
        proba = np.exp(v - lse[:, None]).astype(dtype)
    pred = np.where(bad, -1, np.where(np.isnan(v), -np.inf, v).argmax(axis=1)).astype(np.int64)
    lse[bad], proba[bad] = np.nan, np.nan
    loss = None
    if y is not None:
        y = np.asarray(y, dtype=np.int64)
        ok = (y >= 0) & (y < K)
        loss = np.full(len(v), np.nan, dtype=dtype)
        loss[ok] = lse[ok] - v[ok, y[ok]]
    return lse, loss, pred, proba


def used_rows(x, y, K):
    """the rows sv_probe_accum uses: every entry finite (lse finite) and the label a class"""
    y = np.asarray(y, dtype=np.int64)
    return np.isfinite(np.asarray(x, dtype=np.float64)).all(axis=1) & (y >= 0) & (y < K)


def residuals(x, w, b, y, dtype=np.float64):
    """r [N, K] = exp(v - lse) - [k = y_i]; 0 for a row that is skipped"""
    lse, _, _, proba = rows(x, w, b, None, dtype)
    K = proba.shape[1]
    ok = used_rows(x, y, K)
    r = np.zeros_like(proba)
    hot = np.zeros_like(proba)
    hot[np.nonzero(ok)[0], np.asarray(y, dtype=np.int64)[ok]] = 1
    r[ok] = (proba[ok] - hot[ok]).astype(dtype)
    return r


def margin(x, w, b):
    """the float64 gap between the best and the second-best class of every row"""
    v = np.sort(scores(x, w, b), axis=1)
    return v[:, -1] - v[:, -2]


def allowance(x, w, b, y=None):
    """the 8x rule for v / lse / loss: 8 x the error of the float32 restatement against float64 on these inputs -- and never less than 8
    half ulps of fp32 at the largest result, which no fp32 result can be asked to beat"""
    v64, v32 = scores(x, w, b), scores(x, w, b, np.float32).astype(np.float64)
    r64, r32 = rows(x, w, b, y), rows(x, w, b, y, np.float32)
    pairs = [(v64, v32), (r64[0], r32[0].astype(np.float64))]
    if y is not None:
        pairs.append((r64[1], r32[1].astype(np.float64)))
    err = 0.0
    for a, c in pairs:
        fin = np.isfinite(a) & np.isfinite(c)
        err = max(err, float(np.max(np.abs(a - c)[fin], initial=0.0)))
    return 8.0 * max([err] + [half_ulp32(a) for a, _ in pairs])


# ------------------------------------------------------------------------------------------------ objective and gradient
def pack(w, b):
    """[K, D + 1]: column 0 the intercept, as theta and look"""
    return np.concatenate([np.asarray(b, dtype=np.float64)[:, None], np.asarray(w, dtype=np.float64)], axis=1)


def objective(x, y, t, lam):
    """F(t) = 1/n sum_i (lse_i - v(i, y_i)) + lambda / 2 sum_kd w_kd^2 over the used rows; t = pack(w, b)"""
    t = np.asarray(t, dtype=np.float64)
    ok = used_rows(x, y, t.shape[0])
    _, loss, _, _ = rows(np.asarray(x)[ok], t[:, 1:], t[:, 0], np.asarray(y)[ok])
    return float(loss.mean() + 0.5 * lam * (t[:, 1:] ** 2).sum())


def gradient(x, y, t, lam, dtype=np.float64):
    """the gradient of F at t, [K, D + 1]; dtype: the precision of the scores and residuals (the sums are float64)"""
    t = np.asarray(t, dtype=np.float64)
    ok = used_rows(x, y, t.shape[0])
    xs = np.asarray(x, dtype=np.float64)[ok]
    r = residuals(xs, t[:, 1:], t[:, 0], np.asarray(y)[ok], dtype).astype(np.float64)
    n = float(ok.sum())
    g = np.concatenate([r.sum(axis=0)[:, None], r.T @ xs], axis=1) / n
    g[:, 1:] += lam * t[:, 1:]
    return g


# ------------------------------------------------------------------------------------------------ the partial states
def state_stride(K, D):
    return K * (D + 1) + 1


def accum(x, r, y, lse, loss, P, sums=None, counts=None):
    """sv_probe_accum's partial states from given r [N, K] (the kernel's own, or a restatement's) IN THE KERNEL'S ORDER: tile t of 64
    rows to state t mod P, rows in index order, one float64 add per (row, accumulator), the products r x exact.
    -> (sums float64 [P, K (D + 1) + 1], counts int64 [P, 2]); continues given states"""
    x, r = np.asarray(x, dtype=np.float64), np.asarray(r, dtype=np.float64)
    lse, loss, y = np.asarray(lse, dtype=np.float64), np.asarray(loss, dtype=np.float64), np.asarray(y, dtype=np.int64)
    N, D = x.shape
    K = r.shape[1]
    sums = np.zeros((P, state_stride(K, D))) if sums is None else sums.copy()
    counts = np.zeros((P, 2), dtype=np.int64) if counts is None else counts.copy()
    for i in range(N):
        p = (i // 64) % P
        if not (np.isfinite(lse[i]) and 0 <= y[i] < K):
            counts[p, 1] += 1
            continue
        body = sums[p, :-1].reshape(K, D + 1)
        body[:, 0] += r[i]
        body[:, 1:] += r[i][:, None] * x[i][None, :]
        sums[p, -1] += loss[i]
        counts[p, 0] += 1
    return sums, counts


def merge(sums):
    """the P states added in index order, from 0"""
    total = np.zeros_like(sums[0])
    for s in sums:
        total = total + s
    return total


def _ordered_sum(a):
    """a plain running sum in index order"""
    return float(np.cumsum(np.asarray(a, dtype=np.float64))[-1]) if len(a) else 0.0


def update(sums, counts, K, D, lam, inv_L, beta, theta, look):
    """sv_probe_update in float64, every operation rounded once -> (g [K, D + 1], theta_new, look_new, w fp32, b fp32, stats [4 + 2 K])"""
    theta, look = np.array(theta, dtype=np.float64), np.array(look, dtype=np.float64)
    t = merge(np.asarray(sums, dtype=np.float64))
    n, nskip = int(counts[:, 0].sum()), int(counts[:, 1].sum())
    stats = np.full(4 + 2 * K, np.nan)
    stats[2], stats[3] = n, nskip
    with np.errstate(invalid="ignore", divide="ignore"):
        g = t[:-1].reshape(K, D + 1) / float(n)
    g[:, 1:] = g[:, 1:] + lam * look[:, 1:]
    for k in range(K):
        sq = look[k] * look[k]
        sq[0] = 0.0
        pad = np.zeros(-(-(D + 1) // 256) * 256)
        pad[:D + 1] = sq
        share = np.zeros(256)
        for chunk in pad.reshape(-1, 256):                   # thread t adds its elements t, t + 256, ... in index order
            share = share + chunk
        stats[4 + 2 * k] = np.abs(g[k]).max() if np.isfinite(g[k]).all() else np.nan
        stats[5 + 2 * k] = _ordered_sum(share)
    if n == 0:
        return g, theta, look, look[:, 1:].astype(np.float32), look[:, 0].astype(np.float32), stats
    stats[0] = t[-1] / float(n) + 0.5 * (lam * _ordered_sum(stats[5::2]))
    stats[1] = stats[4::2].max() if np.isfinite(stats[4::2]).all() else np.nan
    tn = look - inv_L * g
    ln = tn + beta * (tn - theta)
    return g, tn, ln, ln[:, 1:].astype(np.float32), ln[:, 0].astype(np.float32), stats


# ------------------------------------------------------------------------------------------------ the fit
def constants(x, y, K, C, standardize=True):
    """what LinearProbe.prepare derives -> (the rows the steps read (fp32 values), mean, scale, lambda, L, beta)"""
    x = np.asarray(x, dtype=np.float64)
    ok = used_rows(x, y, K)
    n = int(ok.sum())
    mean = x[ok].mean(axis=0)
    if standardize:
        sd = np.sqrt(((x[ok] - mean) ** 2).mean(axis=0))
        scale = np.where(sd > 0, sd, 1.0)
        rows_ = ((x - mean) / scale).astype(np.float32).astype(np.float64)
    else:
        mean, scale, rows_ = np.zeros_like(mean), np.ones_like(mean), x
    aug = np.concatenate([rows_[ok], np.ones((n, 1))], axis=1)
    eigmax = float(np.linalg.eigvalsh(aug.T @ aug / n)[-1])
    lam = 1.0 / (C * n)
    lip = 0.5 * eigmax + lam
    q = math.sqrt(lam / lip)
    return rows_, mean, scale, lam, lip, (1.0 - q) / (1.0 + q)


def nesterov(x, y, K, lam, lip, beta, iters, dtype=np.float64, tol=None):
    """`iters` steps of the constant-momentum method from 0 on rows x as given.  dtype float32: the scores and residuals are formed in
    float32 from the look-ahead point rounded to fp32, as the kernels do; the sums and the step are float64 either way.
    -> (theta, look, the max |g| seen at each step's look-ahead point)"""
    D = np.asarray(x).shape[1]
    theta, look, seen = np.zeros((K, D + 1)), np.zeros((K, D + 1)), []
    for _ in range(iters):
        at = look.astype(np.float32).astype(np.float64) if dtype == np.float32 else look
        g = gradient(x, y, at, lam, dtype)
        if dtype == np.float32:
            g[:, 1:] += lam * (look[:, 1:] - at[:, 1:])      # the penalty acts on the double look-ahead point
        seen.append(float(np.abs(g).max()))
        if tol is not None and seen[-1] < tol:
            break
        tn = look - g / lip
        look = tn + beta * (tn - theta)
        theta = tn
    return theta, look, seen


def fit(x, y, K, C=1.0, iters=400, standardize=True, dtype=np.float64):
    """LinearProbe.fit with tol=None -> (w, b of the standardised rows = the look-ahead point, mean, scale, lambda)"""
    rows_, mean, scale, lam, lip, beta = constants(x, y, K, C, standardize)
    _, look, _ = nesterov(rows_, y, K, lam, lip, beta, iters, dtype)
    return look[:, 1:], look[:, 0], mean, scale, lam


def overlapping(n, k, d, seed, spread=1.0, scale=1.5):
    """k overlapping blobs of fp32 values with a common offset and a shear, so that the raw rows are correlated -> (rows, labels)"""
    rng = np.random.default_rng(seed)
    cen = rng.uniform(-scale, scale, (k, d))
    y = np.arange(n) % k
    z = cen[y] + spread * rng.standard_normal((n, d))
    shear = np.eye(d) + 0.3 * np.triu(np.ones((d, d)), 1) / max(1, d - 1)
    return (z @ shear + 3.0).astype(np.float32).astype(np.float64), y.astype(np.int64)
