"""numpy restatement of csrc/aggpost.hip's definitions (include/shotvae_hip.h) in `dtype` arithmetic: float64 is the reference, float32
the kernels' precision -- pair values in fp32 with the 16-block rule, the log-sum-exp in float64 over those fp32 values, and the result
rounded once to fp32, the type of the kernels' outputs (lqx, lpz and the densities; returned as float64 arrays).  The normal
stream is tests/_score_ref.py's.  Two input recipes: `spread` (tests/_knn_ref.posterior: one gallery row carries each sum) and `overlap`
(nearly coincident posteriors: many rows carry it -- a kernel that returned the largest term would fail on it).  numpy only."""
import math

import numpy as np

from tests import _knn_ref as KR
from tests import _score_ref as SR

HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
RECIPES = ("spread", "overlap")
MIN_ESS = 8.0


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def spread(n, d, stream):
    return KR.posterior(n, d, stream)


def overlap(n, d, stream):
    """ls = base_d + 0.01 U(-1, 1), mu = 0.1 exp(base_d) N(0, 1), base_d ~ U(-1, 0.5) -- base_d depends on d alone, so that rows of
    different streams overlap too; fp32 values as float64 arrays"""
    from oracle import closed_form as C
    base = C.uniform((1, d), 9800, -1.0, 0.5).numpy().astype(np.float64)
    ls = base + 0.01 * C.uniform((n, d), stream + 1, -1.0, 1.0).numpy().astype(np.float64)
    mu = 0.1 * np.exp(base) * C.normal((n, d), stream).numpy().astype(np.float64)
    return mu.astype(np.float32).astype(np.float64), ls.astype(np.float32).astype(np.float64)


def rows(recipe, n, d, stream):
    return {"spread": spread, "overlap": overlap}[recipe](n, d, stream)


def queries(recipe, n, d, stream, key=77):
    """z [n, d]: one draw from each of n posteriors of the recipe (fp32 values as float64)"""
    mu, ls = rows(recipe, n, d, stream)
    return sample(mu, ls, key, 0, 0, np.float32)[0].astype(np.float64)


def _out(a, dtype):
    """an output of the kernels is fp32: the float32 restatement rounds its float64 result once"""
    return a.astype(np.float32).astype(np.float64) if dtype == np.float32 else a


# ---- sv_aggpost_sample -----------------------------------------------------------------------------------------------------------
def sample(mu, ls, key, row0, s, dtype=np.float64):
    """(z [Q, D] in dtype, lqx [Q], lpz [Q] float64): terms in `dtype`, sums in float64"""
    Q, D = mu.shape
    m, l = mu.astype(dtype), ls.astype(dtype)
    n = np.zeros((Q, D), dtype) if key is None else SR.sweep_normals(key, row0, Q, 1, D, dtype, s0=s)[:, 0, :]
    z = m if key is None else m + np.exp(l) * n
    lqx = (dtype(-0.5) * n * n - l).astype(np.float64).sum(axis=1) - D * HALF_LOG_2PI
    lpz = (dtype(-0.5) * z * z).astype(np.float64).sum(axis=1) - D * HALF_LOG_2PI
    return z, _out(lqx, dtype), _out(lpz, dtype)


# ---- the pair values -------------------------------------------------------------------------------------------------------------
def pair_values(z, mu, ls, dtype=np.float64):
    """v [Q, N] float64: log N(z_i; mu_j, sigma_j^2); float32: 16 dimensions summed in fp32 in index order, the blocks in float64"""
    z, mu_, ls_ = (np.asarray(a, dtype) for a in (z, mu, ls))
    Q, D = z.shape
    with np.errstate(invalid="ignore", over="ignore"):
        b = np.exp(dtype(-2) * ls_)
        acc = np.zeros((Q, mu_.shape[0]), np.float64)
        for d0 in range(0, D, 16):
            part = np.zeros((Q, mu_.shape[0]), dtype)
            for d in range(d0, min(d0 + 16, D)):
                dm = z[:, None, d] - mu_[None, :, d]
                part = part + (dm * dm) * b[None, :, d]
            acc += part.astype(np.float64)
        return -0.5 * acc - ls_.astype(np.float64).sum(axis=1)[None, :] - D * HALF_LOG_2PI


def dim_values(z, mu, ls, dtype=np.float64):
    """v_d [Q, N, D] in dtype"""
    z, mu_, ls_ = (np.asarray(a, dtype) for a in (z, mu, ls))
    with np.errstate(invalid="ignore", over="ignore"):
        dm = z[:, None, :] - mu_[None, :, :]
        return (dm * dm) * (dtype(-0.5) * np.exp(dtype(-2) * ls_))[None] + (-ls_ - dtype(HALF_LOG_2PI))[None]


# ---- the log-sum-exp state -------------------------------------------------------------------------------------------------------
def state(v, axis=1):
    """(m, s) of the terms v along `axis` (float64): m the maximum, s = sum exp(v - m); empty / all -inf: (-inf, 0); NaN: (NaN, 0)"""
    v = np.asarray(v, np.float64)
    if v.shape[axis] == 0:
        shape = tuple(n for i, n in enumerate(v.shape) if i != axis)
        return np.full(shape, -np.inf), np.zeros(shape)
    nan = np.isnan(v).any(axis=axis)
    with np.errstate(invalid="ignore"):
        m = np.where(nan, np.nan, np.max(np.where(np.isnan(v), -np.inf, v), axis=axis))
        fin = np.isfinite(m)
        safe = np.where(fin, m, 0.0)
        s = np.where(fin, np.exp(v - np.expand_dims(safe, axis)).sum(axis=axis), np.where(m == np.inf, 1.0, 0.0))
    return m, np.where(nan, 0.0, s)


def finish(ms, ss, count):
    """sv_aggpost_finish: states m, s [P, ...] -> M + log(sum_p s_p exp(m_p - M)) - log(count)"""
    ms, ss = np.asarray(ms, np.float64), np.asarray(ss, np.float64)
    nan = np.isnan(ms).any(axis=0) | np.isnan(ss).any(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        M = np.max(np.where(np.isnan(ms), -np.inf, ms), axis=0)
        fin = np.isfinite(M)
        safe = np.where(fin, M, 0.0)
        w = np.where(ms > -np.inf, ss * np.exp(np.where(ms > -np.inf, ms, 0.0) - safe[None]), 0.0)
        out = np.where(fin, safe + np.log(w.sum(axis=0)) - math.log(count), M)
    return np.where(nan, np.nan, out)


def _drop_self(v, col0, self0):
    if self0 >= 0:
        v = v.copy()
        for i in range(v.shape[0]):
            r = self0 + i - col0
            if 0 <= r < v.shape[1]:
                v[i, r] = -np.inf
    return v


def log_density(z, mu, ls, dtype=np.float64, self0=-1, count=None):
    """lq [Q]: the joint density's log mean over the gallery (row self0 + i left out for query i when self0 >= 0)"""
    v = _drop_self(pair_values(z, mu, ls, dtype), 0, self0)
    m, s = state(v, 1)
    return _out(finish(m[None], s[None], count or (v.shape[1] - (self0 >= 0))), dtype)


def log_density_dims(z, mu, ls, dtype=np.float64, self0=-1, count=None):
    """lq_d [Q, D]"""
    v = dim_values(z, mu, ls, dtype).astype(np.float64)
    if self0 >= 0:
        for i in range(v.shape[0]):
            if 0 <= self0 + i < v.shape[1]:
                v[i, self0 + i, :] = -np.inf
    m, s = state(v, 1)
    return _out(finish(m[None], s[None], count or (v.shape[1] - (self0 >= 0))), dtype)


def min_ess(z, mu, ls):
    """the smallest effective number of contributing terms 1 / sum w^2 over the queries, w the normalised weights (float64)"""
    v = pair_values(z, mu, ls)
    w = np.exp(v - v.max(axis=1, keepdims=True))
    w /= w.sum(axis=1, keepdims=True)
    return float((1.0 / (w * w).sum(axis=1)).min())


# ---- the 8x rule -----------------------------------------------------------------------------------------------------------------
_TOL = {}


def tolerance_for(kind, recipe, D, N=64):
    """8 x the largest error of the float32 restatement against the float64 one on 64 x 64 rows of the recipe: kind "scan" (lq),
    "dims" (lq_d), "pair" (a single pair value), "sample" ((z, lqx, lpz) -> three allowances).  A density over a gallery of N < 64
    rows averages over fewer terms than one over 64 -- at N = 1 it IS a pair value, far pairs included, whose fp32 error is that of
    a number of the pair's magnitude --, so for N < 64 the 64 gallery rows are cut into galleries of N rows and the error is the
    largest over all of them (N >= 64: the one gallery of 64 rows)."""
    n = min(int(N), 64)
    k = (kind, recipe, D, n)
    if k not in _TOL:
        mu, ls = rows(recipe, 64, D, 9990)
        if kind == "sample":
            a, b = sample(mu, ls, 5, 0, 0, np.float32), sample(mu, ls, 5, 0, 0, np.float64)
            _TOL[k] = tuple(8.0 * float(np.abs(np.asarray(x, np.float64) - y).max()) for x, y in zip(a, b))
        else:
            z = queries(recipe, 64, D, 9992)
            fn = {"scan": log_density, "dims": log_density_dims, "pair": pair_values}[kind]
            cuts = [(0, 64)] if kind == "pair" else [(a, a + n) for a in range(0, 64 - n + 1, n)]
            _TOL[k] = 8.0 * max(float(np.abs(fn(z, mu[a:b], ls[a:b], np.float32) - fn(z, mu[a:b], ls[a:b], np.float64)).max())
                                for a, b in cuts)
    return _TOL[k]


# ---- evaluate_aggregate ----------------------------------------------------------------------------------------------------------
def entropy(q):
    q = np.asarray(q, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return -np.where(q > 0, q * np.log(q), 0.0).sum(axis=-1)


def diagnostics(g_mu, g_ls, qy, samples=1, key=0, q_mu=None, q_ls=None, per_dim=True, dtype=np.float64):
    """evaluate_aggregate restated on encoded posteriors: gallery (g_mu, g_ls) [N, D], q(y | x) qy [N, K]; the queries default to the
    gallery; query i draws from row0 + i = i"""
    q_mu, q_ls = (g_mu, g_ls) if q_mu is None else (q_mu, q_ls)
    N, D = g_mu.shape
    Q = q_mu.shape[0]
    lqx = lq = lpz = lqd = 0.0
    dim = np.zeros(D)
    for s in range(samples):
        z, a, c = sample(q_mu, q_ls, key, 0, s, dtype)
        z = np.asarray(z, np.float64)
        b = log_density(z, g_mu, g_ls, dtype)
        lqx, lq, lpz = lqx + a.sum(), lq + b.sum(), lpz + c.sum()
        if per_dim:
            d = log_density_dims(z, g_mu, g_ls, dtype)
            lqd += d.sum()
            dim += (d + 0.5 * z * z + HALF_LOG_2PI).sum(axis=0)
    n = float(Q * samples)
    lqx, lq, lpz, lqd = lqx / n, lq / n, lpz / n, lqd / n
    qbar = np.asarray(qy, np.float64).mean(axis=0)
    res = dict(mi=lqx - lq, marginal_kl=lq - lpz, kl_c_mc=lqx - lpz,
               kl_c=float((0.5 * (q_mu * q_mu + np.exp(2.0 * q_ls) - 2.0 * q_ls - 1.0)).sum() / Q), log_n=math.log(N),
               active_units=int((np.var(g_mu, axis=0) > 0.01).sum()), mi_y=float(entropy(qbar) - entropy(qy).mean()),
               marginal_kl_y=float(math.log(len(qbar)) - entropy(qbar)))
    if per_dim:
        res.update(total_correlation=lq - lqd, dim_kl=dim / n, dimwise_kl=float(dim.sum() / n))
    return res
