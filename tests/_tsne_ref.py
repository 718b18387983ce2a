"""numpy float64 restatement of csrc/tsne.hip's and shot_vae_amd/embed.py's definitions (include/shotvae_hip.h): the
bisection for beta with the invalid-slot rule, the dense symmetric P, the attraction A, the repulsion R, Z, the KL and the gradient,
the update with gains and momentum, and a whole run.  tests/test_tsne_cpu.py pins it to scikit-learn and to finite differences; the GPU
tests measure their allowances with it: `dtype=np.float32` gives the fp32 restatement the 8x rule needs (every pair value in fp32, the
sums over the columns one add per column in column order, as the kernels take them)."""
import math

import numpy as np


# ---------------------------------------------------------------------------------------------- input affinities
def valid_slots(dist, idx):
    return (np.asarray(idx) >= 0) & np.isfinite(np.asarray(dist, dtype=np.float64))


def softmax_row(d, ok, beta):
    """p over the valid slots of one row at `beta`, float64 (0 on the others); exp(0) for the closest slot whatever beta"""
    d = np.asarray(d, dtype=np.float64)
    p = np.zeros(len(d))
    if not ok.any():
        return p
    x = d[ok] - d[ok].min()
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.where(x == 0.0, 1.0, np.exp(-beta * x))
    p[ok] = e / e.sum()
    return p


def entropy(p):
    """the Shannon entropy in nats, 0 log 0 = 0"""
    p = np.asarray(p, dtype=np.float64)
    p = p[p > 0]
    return float(-(p * np.log(p)).sum())


def search_row(d, ok, perplexity, tol=1e-5, max_steps=100):
    """scikit-learn's bisection for one row -> (p float64 [k], beta, steps): at most max_steps evaluations of H; steps = the number of
    evaluations when |H - log(perplexity)| <= tol was met, max_steps when it never was; beta is not moved after the last evaluation"""
    d = np.asarray(d, dtype=np.float64)
    if ok.sum() < 2:
        return np.where(ok, 1.0, 0.0), 1.0, max_steps
    x = d[ok] - d[ok].min()
    target = math.log(perplexity)
    beta, lo, hi = 1.0, -math.inf, math.inf
    steps = max_steps
    for it in range(max_steps):
        with np.errstate(over="ignore", invalid="ignore"):
            e = np.where(x == 0.0, 1.0, np.exp(-beta * x))
        S, T = e.sum(), (x * e).sum()
        H = math.log(S) + (0.0 if T == 0.0 else beta * (T / S))
        diff = H - target
        if abs(diff) <= tol:
            steps = it + 1
            break
        if it + 1 == max_steps:
            break
        if diff > 0.0:
            lo = beta
            beta = beta * 2.0 if hi == math.inf else 0.5 * (beta + hi)
        else:
            hi = beta
            beta = beta * 0.5 if lo == -math.inf else 0.5 * (beta + lo)
    p = np.zeros(len(d))
    p[ok] = e / S
    return p, beta, steps


def conditional(dist, idx, perplexity, tol=1e-5, max_steps=100):
    """-> (p float64 [N, k], beta float64 [N], steps int [N])"""
    dist = np.asarray(dist, dtype=np.float64)
    ok = valid_slots(dist, idx)
    rows = [search_row(dist[i], ok[i], perplexity, tol, max_steps) for i in range(len(dist))]
    return np.stack([r[0] for r in rows]), np.array([r[1] for r in rows]), np.array([r[2] for r in rows], dtype=np.int64)


def joint_dense(p, idx):
    """the dense symmetric P [N, N] = (P_cond + P_cond^T) / (2N) of the conditional p [N, k] on the lists idx (idx < 0: no edge)"""
    p, idx = np.asarray(p, dtype=np.float64), np.asarray(idx)
    n = len(p)
    cond = np.zeros((n, n))
    for i in range(n):
        for j, v in zip(idx[i], p[i]):
            if j >= 0:
                cond[i, j] += v
    return (cond + cond.T) / (2.0 * n)


# ---------------------------------------------------------------------------------------------- the low-dimensional side
def repulsion(y, dtype=np.float64):
    """(R [N, d], Z_i [N]) in `dtype`: R_i = sum_{j != i} w_ij^2 (y_i - y_j), Z_i = sum_{j != i} w_ij, one add per column in column
    order; the pair is left out by index (duplicates count 1 each into Z)"""
    y = np.asarray(y, dtype=dtype)
    n, d = y.shape
    R, Z = np.zeros((n, d), dtype=dtype), np.zeros(n, dtype=dtype)
    one = dtype(1.0)
    for j in range(n):
        df = y - y[j]
        r2 = df[:, 0] * df[:, 0]
        for c in range(1, d):
            r2 = r2 + df[:, c] * df[:, c]
        w = one / (one + r2)
        w[j] = 0
        Z = Z + w
        R = R + (w * w)[:, None] * df
    return R, Z


def pair_sq(y, dtype=np.float64):
    y = np.asarray(y, dtype=dtype)
    df = y[:, None, :] - y[None, :, :]
    r2 = df[:, :, 0] * df[:, :, 0]
    for c in range(1, y.shape[1]):
        r2 = r2 + df[:, :, c] * df[:, :, c]
    return df, r2


def attraction(P, y, dtype=np.float64):
    """(A [N, d], rowkl [N]) of the dense P in `dtype`: A_i = sum_j P_ij w_ij (y_i - y_j), rowkl_i = sum_{P_ij > 0} P_ij log(P_ij (1 + r2_ij))"""
    P = np.asarray(P, dtype=dtype)
    df, r2 = pair_sq(y, dtype)
    one = dtype(1.0)
    A = ((P * (one / (one + r2)))[:, :, None] * df).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(P > 0, P * np.log(np.where(P > 0, P, one) * (one + r2)), dtype(0.0))
    return A, t.sum(axis=1)


def gradient(P, y, exaggeration=1.0):
    """float64 -> (g [N, d] = 4 (e A - R / Z), KL of the UNEXAGGERATED P, Z)"""
    A, rowkl = attraction(P, y)
    R, Zi = repulsion(y)
    Z = float(Zi.sum())
    return 4.0 * (exaggeration * A - R / Z), float(rowkl.sum() + math.log(Z)), Z


def kl(P, y):
    return gradient(P, y)[1]


def update(y, vel, gain, g, momentum, lr):
    """scikit-learn's _gradient_descent step per element -> (y, vel, gain); no recentring"""
    inc = vel * g < 0.0
    gain = np.maximum(np.where(inc, gain + 0.2, gain * 0.8), 0.01)
    vel = momentum * vel - lr * gain * g
    return y + vel, vel, gain


def run(P, y0, n_iter, exaggeration_iter, early_exaggeration, lr):
    """the whole schedule in float64 from y0 -> (y, the KL of every iteration's starting point)"""
    y = np.asarray(y0, dtype=np.float64).copy()
    vel, gain = np.zeros_like(y), np.ones_like(y)
    kls = []
    for it in range(n_iter):
        early = it < exaggeration_iter
        g, k, _ = gradient(P, y, early_exaggeration if early else 1.0)
        kls.append(k)
        y, vel, gain = update(y, vel, gain, g, 0.5 if early else 0.8, lr)
    return y, kls


def one_nn_hit(y, labels):
    """the leave-one-out 1-NN label accuracy of the embedding (ties by the smaller index)"""
    _, r2 = pair_sq(y)
    np.fill_diagonal(r2, np.inf)
    return float((np.asarray(labels)[np.argmin(r2, axis=1)] == np.asarray(labels)).mean())


def knn_lists(x, k):
    """(dist [N, k], idx [N, k]) of the squared Euclid distance, self excluded, closest first, ties by the smaller index"""
    _, r2 = pair_sq(x)
    np.fill_diagonal(r2, np.inf)
    idx = np.argsort(r2, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(r2, idx, axis=1), idx.astype(np.int64)


def outcome_case(n, classes, dim, k, perplexity, jitter=0.0, seed=0):
    """the blobs of tests/_cluster_ref.py, their k-lists, the dense P and the PCA start (+ a perturbation) -> (P, y0, labels)"""
    import torch
    from shot_vae_amd import pca_project
    from tests import _cluster_ref as CR
    x, _, which = CR.blobs(n, classes, dim, 9100 + n)
    dist, idx = knn_lists(x, k)
    P = joint_dense(conditional(dist.astype(np.float32), idx, perplexity)[0], idx)
    y0 = pca_project(torch.from_numpy(x), 2).numpy()
    if jitter:
        y0 = y0 + jitter * np.random.default_rng(seed).normal(size=y0.shape)
    return P, y0, which
