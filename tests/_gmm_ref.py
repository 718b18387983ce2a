"""Diagonal Gaussian mixtures restated in numpy from the header comments of include/shotvae_hip.h (sv_gmm_*): the value of a pair, the
table, the E-step, the partial states in the kernel's own order, scikit-learn's M-step and the sampler's stream, each in float64 (the
reference) or float32 (the kernels' own precision, for the 8x rule).  numpy only: shared by tests/test_gmm_cpu.py (which pins it to
scikit-learn) and tests/test_gmm_gpu.py."""
import math
import os
import re

import numpy as np

from tests._score_ref import philox4x32_10

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = 10.0 * np.finfo(np.float64).eps


def gmm_tag():
    """SV_GMM_PHILOX_TAG of the header"""
    with open(os.path.join(ROOT, "include", "shotvae_hip.h")) as f:
        return int(re.search(r"#define\s+SV_GMM_PHILOX_TAG\s+(0x[0-9A-Fa-f]+)u", f.read()).group(1), 16)


def all_tags():
    with open(os.path.join(ROOT, "include", "shotvae_hip.h")) as f:
        return {n: int(v, 16) for n, v in re.findall(r"#define\s+(SV_\w+_PHILOX_TAG)\s+(0x[0-9A-Fa-f]+)u", f.read())}


# ------------------------------------------------------------------------------------------------ the table and the pair
def prepare(logw, mean, var, dtype=np.float64):
    """-> (ivar [K, D], cst [K], cdf [K]) of sv_gmm_prepare"""
    logw, var = np.asarray(logw, dtype=dtype), np.asarray(var, dtype=dtype)
    D = var.shape[1]
    with np.errstate(divide="ignore"):
        cst = logw - dtype(0.5) * (dtype(D * math.log(2.0 * math.pi)) + np.log(var).sum(axis=1, dtype=dtype))
    w = np.exp(logw.astype(np.float64))
    cdf = np.cumsum(w) / w.sum()
    if (w > 0).any():
        cdf[np.nonzero(w > 0)[0][-1]] = 1.0
    return (dtype(1) / var).astype(dtype), cst.astype(dtype), cdf.astype(dtype)


def pair_values(x, logw, mean, var, dtype=np.float64):
    """v [N, K]: cst_k - 1/2 sum_d (x - mean)^2 ivar; -inf for a component of weight 0; NaN for a row that is not finite"""
    x, mean = np.asarray(x, dtype=dtype), np.asarray(mean, dtype=dtype)
    ivar, cst, _ = prepare(logw, mean, var, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        q = (((x[:, None, :] - mean[None, :, :]) ** 2) * ivar[None, :, :]).sum(axis=2, dtype=dtype)
        v = cst[None, :] - dtype(0.5) * q
    v = np.where(np.isneginf(cst)[None, :], -np.inf, v)
    v[~np.isfinite(x).all(axis=1)] = np.nan
    return v.astype(dtype)


def estep(x, logw, mean, var, dtype=np.float64):
    """-> (lse [N], assign int64 [N], resp [N, K]) of sv_gmm_estep"""
    v = pair_values(x, logw, mean, var, dtype)
    bad = np.isnan(v).any(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.where(bad, 0.0, v.max(axis=1))
        m = np.where(np.isfinite(m), m, 0.0).astype(dtype)
        lse = m + np.log(np.exp(v - m[:, None]).sum(axis=1, dtype=dtype))
        resp = np.exp(v - lse[:, None])
    fin = np.where(np.isfinite(v), v, -np.inf)
    assign = fin.argmax(axis=1).astype(np.int64)
    assign[bad | ~np.isfinite(fin).any(axis=1)] = -1
    lse[bad], resp[bad] = np.nan, np.nan
    return lse.astype(dtype), assign, resp.astype(dtype)


def half_ulp32(a):
    a = np.asarray(a, dtype=np.float64)
    a = a[np.isfinite(a)]
    return 0.5 * float(np.spacing(np.float32(np.abs(a).max()))) if a.size else 0.0


def allowance(x, logw, mean, var):
    """the 8x rule for lse / v: 8 x the error of the float32 restatement against float64 on these inputs -- and never less than 8 half
    ulps of fp32 at the largest result, which no fp32 result can be asked to beat"""
    v64, v32 = pair_values(x, logw, mean, var), pair_values(x, logw, mean, var, np.float32).astype(np.float64)
    l64, l32 = estep(x, logw, mean, var)[0], estep(x, logw, mean, var, np.float32)[0].astype(np.float64)
    err = 0.0
    for a, b in ((v64, v32), (l64, l32)):
        fin = np.isfinite(a) & np.isfinite(b)
        err = max(err, float(np.max(np.abs(a - b)[fin], initial=0.0)))
    return 8.0 * max(err, half_ulp32(v64), half_ulp32(l64))


def margin(x, logw, mean, var):
    """the float64 gap between the best and the second-best component of every row"""
    v = np.sort(np.where(np.isfinite(pair_values(x, logw, mean, var)), pair_values(x, logw, mean, var), -np.inf), axis=1)
    return v[:, -1] - v[:, -2] if v.shape[1] > 1 else np.full(len(v), np.inf)


# ------------------------------------------------------------------------------------------------ the M-step
def mstep(x, resp, reg_covar):
    """scikit-learn's M-step for covariance_type="diag" -> (n_k, logw, mean, var)"""
    x, resp = np.asarray(x, dtype=np.float64), np.asarray(resp, dtype=np.float64)
    nk = resp.sum(axis=0) + TINY
    mean = resp.T @ x / nk[:, None]
    var = resp.T @ (x * x) / nk[:, None] - mean ** 2 + reg_covar
    return nk, np.log(nk / nk.sum()), mean, var


def em_step(x, logw, mean, var, reg_covar):
    """one EM iteration -> (logw, mean, var, the lower bound at the parameters the step started from)"""
    lse, _, resp = estep(x, logw, mean, var)
    _, lw, m, v = mstep(x, resp, reg_covar)
    return lw, m, v, float(lse.mean())


def state_stride(K, D):
    return K * (2 * D + 1) + 1


def accum(x, r, lse, P, sums=None, counts=None):
    """sv_gmm_accum's partial states from given r [N, K] (the kernel's own, or a restatement's) IN THE KERNEL'S ORDER: tile t of 64 rows to
    state t mod P, rows in index order, one float64 add per (row, accumulator), the products (r x) exact and ((r x) x) rounded first.
    -> (sums float64 [P, K (2 D + 1) + 1], counts int64 [P, 2]); continues given states"""
    x, r, lse = np.asarray(x, dtype=np.float64), np.asarray(r, dtype=np.float64), np.asarray(lse, dtype=np.float64)
    N, D = x.shape
    K = r.shape[1]
    sums = np.zeros((P, state_stride(K, D))) if sums is None else sums.copy()
    counts = np.zeros((P, 2), dtype=np.int64) if counts is None else counts.copy()
    for i in range(N):
        p = (i // 64) % P
        if not np.isfinite(lse[i]):
            counts[p, 1] += 1
            continue
        body = sums[p, :-1].reshape(K, 2 * D + 1)
        rx = r[i][:, None] * x[i][None, :]
        body[:, 0] += r[i]
        body[:, 1:D + 1] += rx
        body[:, D + 1:] += rx * x[i][None, :]
        sums[p, -1] += lse[i]
        counts[p, 0] += 1
    return sums, counts


def merge(sums):
    """the P states added in index order"""
    total = np.zeros_like(sums[0])
    for s in sums:
        total = total + s
    return total


def finish(sums, counts, K, D, reg_covar, logw, mean, var):
    """sv_gmm_finish in float64 -> (logw, mean, var, stats [4])"""
    t = merge(np.asarray(sums, dtype=np.float64))
    body = t[:-1].reshape(K, 2 * D + 1)
    raw = body[:, 0]
    live = raw != 0.0
    nk = raw + TINY
    mean, var = np.array(mean, dtype=np.float64), np.array(var, dtype=np.float64)
    m = body[:, 1:D + 1] / nk[:, None]
    v = body[:, D + 1:] / nk[:, None] - m * m + reg_covar
    mean[live], var[live] = m[live], v[live]
    with np.errstate(divide="ignore"):
        lw = np.where(live, np.log(nk / nk[live].sum()), -np.inf)
    nfin, nskip = int(counts[:, 0].sum()), int(counts[:, 1].sum())
    stats = np.array([t[-1] / nfin if nfin else np.nan, nfin, nskip, var[live].min() if live.any() else np.inf])
    return lw, mean, var, stats


def n_parameters(K, D):
    return K - 1 + 2 * K * D


# ------------------------------------------------------------------------------------------------ the sampler
def _rows(row0, B):
    rows = np.arange(B, dtype=np.uint64) + np.uint64(row0)
    return (rows & np.uint64(0xFFFFFFFF)).astype(np.uint32), (rows >> np.uint64(32)).astype(np.uint32)


def sample_uniform(key, row0, B, tag=None):
    """u of rows row0 .. row0 + B - 1: (r[0] >> 8) 2^-24 of the generator call whose third counter word is 0xFFFFFFFF"""
    k = int(key) & 0xFFFFFFFFFFFFFFFF
    lo, hi = _rows(row0, B)
    r = philox4x32_10(lo, hi, np.uint32(0xFFFFFFFF) + 0 * lo, np.uint32(gmm_tag() if tag is None else tag), np.uint32(k & 0xFFFFFFFF),
                      np.uint32(k >> 32))
    return (r[0] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def sample_normals(key, row0, B, D, dtype=np.float64, tag=None):
    """n(row0 + b, d): sv_latent_draw's counter and Box-Muller mapping under the mixture's tag"""
    k = int(key) & 0xFFFFFFFFFFFFFFFF
    lo, hi = (a[:, None] for a in _rows(row0, B))
    nj = (D + 3) // 4
    j = np.arange(nj, dtype=np.uint32)[None, :]
    r = philox4x32_10(lo + 0 * j, hi + 0 * j, j + 0 * lo, np.uint32(gmm_tag() if tag is None else tag), np.uint32(k & 0xFFFFFFFF),
                      np.uint32(k >> 32))
    out = np.empty((B, 4 * nj), dtype=dtype)
    for p in range(2):
        u1 = (((r[2 * p] >> np.uint32(8)).astype(np.int64) + 1).astype(dtype)) * dtype(2.0 ** -24)
        u2 = (r[2 * p + 1] >> np.uint32(8)).astype(dtype) * dtype(2.0 ** -24)
        rad = np.sqrt(dtype(-2.0) * np.log(u1))
        ang = dtype(2.0 * math.pi) * u2
        out[:, 2 * p::4] = rad * np.cos(ang)
        out[:, 2 * p + 1::4] = rad * np.sin(ang)
    return out[:, :D]


def choose(cdf, u):
    """the first k with cdf_k > u; K - 1 if there is none"""
    cdf, u = np.asarray(cdf), np.asarray(u)
    hit = cdf[None, :] > u[:, None]
    return np.where(hit.any(axis=1), hit.argmax(axis=1), len(cdf) - 1).astype(np.int64)


def sample(key, row0, B, mean, var, cdf, dtype=np.float64):
    """-> (z [B, D], comp int64 [B]) of sv_gmm_sample; cdf: the fp32 table the kernel reads"""
    comp = choose(np.asarray(cdf, dtype=np.float32).astype(np.float64), sample_uniform(key, row0, B))
    mean, var = np.asarray(mean, dtype=dtype), np.asarray(var, dtype=dtype)
    n = sample_normals(key, row0, B, mean.shape[1], dtype)
    return mean[comp] + np.sqrt(var[comp]) * n, comp


# ------------------------------------------------------------------------------------------------ inputs
def blobs(n, k, d, seed, spread=0.25, scale=4.0):
    """k separated blobs -> (rows [n, d] of fp32 values, centres [k, d], the blob of every row)"""
    rng = np.random.default_rng(seed)
    cen = np.round(rng.uniform(-scale, scale, (k, d)) * 4.0) / 4.0 + scale * 3.0 * np.eye(k, d)
    which = np.arange(n) % k
    rows = (cen[which] + spread * rng.standard_normal((n, d))).astype(np.float32).astype(np.float64)
    return rows, cen, which


def model(k, d, seed, var_lo=0.25, var_hi=2.0, scale=2.0):
    """a random mixture of fp32 values -> (logw, mean, var)"""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.5, 1.5, k)
    f = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)          # noqa: E731
    return f(np.log(w / w.sum())), f(rng.uniform(-scale, scale, (k, d))), f(rng.uniform(var_lo, var_hi, (k, d)))
