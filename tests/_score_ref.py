"""The per-image scores restated in numpy, from the header comments of include/shotvae_hip.h: sv_latent_sweep's normal stream, z and lw,
sv_recon_rows' term and sv_score_reduce's formulas, each in float64 (the reference) or float32 (the kernels' own precision).  numpy
only: shared by tests/test_score_cpu.py, tests/test_score_gpu.py and the fixture generator tests/golden/make_score_goldens.py."""
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox-4x32-10 (Salmon et al., SC'11) on uint32 arrays (broadcast); returns the four output words"""
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint32) for v in (c0, c1, c2, c3))
    k0, k1 = np.asarray(k0, dtype=np.uint32), np.asarray(k1, dtype=np.uint32)
    with np.errstate(over="ignore"):
        for r in range(10):
            if r:
                k0, k1 = k0 + W0, k1 + W1
            p0, p1 = M0 * c0.astype(np.uint64), M1 * c2.astype(np.uint64)
            h0, l0 = (p0 >> np.uint64(32)).astype(np.uint32), p0.astype(np.uint32)
            h1, l1 = (p1 >> np.uint64(32)).astype(np.uint32), p1.astype(np.uint32)
            c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
    return c0, c1, c2, c3


def score_tag():
    """SV_SCORE_PHILOX_TAG of the header"""
    with open(os.path.join(ROOT, "include", "shotvae_hip.h")) as f:
        return int(re.search(r"#define\s+SV_SCORE_PHILOX_TAG\s+(0x[0-9A-Fa-f]+)u", f.read()).group(1), 16)


def sweep_normals(key, row0, B, S, ldc, dtype=np.float64, s0=0):
    """n(row0 + b, s0 + s, d) of sv_latent_sweep for b < B, s < S, d < ldc -> [B, S, ldc], restated from the header comment in
    `dtype` arithmetic (float64: the reference; float32: the kernel's own precision).  The uniforms are exact in either."""
    k = int(key) & 0xFFFFFFFFFFFFFFFF
    rows = (np.arange(B, dtype=np.uint64) + np.uint64(row0))[:, None, None]
    nj = (ldc + 3) // 4
    c2 = ((np.arange(S, dtype=np.uint32) + np.uint32(s0)) << np.uint32(16))[None, :, None] | np.arange(nj, dtype=np.uint32)[None, None, :]
    lo, hi = (rows & np.uint64(0xFFFFFFFF)).astype(np.uint32), (rows >> np.uint64(32)).astype(np.uint32)
    r = philox4x32_10(lo + 0 * c2, hi + 0 * c2, c2 + 0 * lo, np.uint32(score_tag()), np.uint32(k & 0xFFFFFFFF), np.uint32(k >> 32))
    out = np.empty((B, S, 4 * nj), dtype=dtype)
    for p in range(2):
        u1 = (((r[2 * p] >> np.uint32(8)).astype(np.int64) + 1).astype(dtype)) * dtype(2.0 ** -24)
        u2 = (r[2 * p + 1] >> np.uint32(8)).astype(dtype) * dtype(2.0 ** -24)
        rad = np.sqrt(dtype(-2.0) * np.log(u1))
        ang = dtype(2.0 * math.pi) * u2
        out[:, :, 2 * p::4] = rad * np.cos(ang)
        out[:, :, 2 * p + 1::4] = rad * np.sin(ang)
    return out[:, :, :ldc]


def sweep_z(key, row0, B, S, ldc, mu, ls, dtype=np.float64):
    """z [B, S, ldc] of sv_latent_sweep in `dtype` arithmetic; key None: z = mu"""
    m = mu.astype(dtype)[:, None, :]
    if key is None:
        return np.broadcast_to(m, (B, S, ldc)).copy()
    return m + np.exp(ls.astype(dtype))[:, None, :] * sweep_normals(key, row0, B, S, ldc, dtype)


def sweep_lw(key, row0, B, S, ldc, mu, ls, dtype=np.float64):
    """lw [B, S] = sum_d (n^2 / 2 - z^2 / 2 + ls)"""
    n = np.zeros((B, S, ldc), dtype) if key is None else sweep_normals(key, row0, B, S, ldc, dtype)
    z = sweep_z(key, row0, B, S, ldc, mu, ls, dtype)
    return (dtype(0.5) * n * n - dtype(0.5) * z * z + ls.astype(dtype)[:, None, :]).sum(axis=2, dtype=dtype)


def nll_rows(r, x, bce, x_sigma=1.0, dtype=np.float64):
    """sv_recon_rows' term of logits r [R, C, H, W] against images x (same shape), per row"""
    r, x = r.astype(dtype), x.astype(dtype)
    if bce:
        t = np.maximum(r, dtype(0)) - r * x + np.log1p(np.exp(-np.abs(r)))
        return t.reshape(len(r), -1).sum(axis=1, dtype=dtype)
    with np.errstate(over="ignore"):
        e = dtype(1) / (dtype(1) + np.exp(-r)) - x
    return (e * e).reshape(len(r), -1).sum(axis=1, dtype=dtype) * dtype(1.0 / (2.0 * x_sigma * x_sigma))


def lse(a, axis, dtype=np.float64):
    """log-sum-exp about the maximum: -inf terms have weight 0, an all -inf slice gives -inf, a +inf term gives +inf, a NaN term NaN"""
    a = np.asarray(a, dtype)
    m = a.max(axis=axis, keepdims=True)
    safe = np.where(np.isfinite(m), m, dtype(0))
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.log(np.exp(a - safe).sum(axis=axis, keepdims=True, dtype=dtype)) + safe
    return np.where(np.isfinite(m), v, m).squeeze(axis)


def ref_scores(nll, lw, la, mu, ls, add=0.0, dtype=np.float64):
    """sv_score_reduce restated: nll [B, S, Kd] (Kd = K or 1), lw [B, S], la [B, K], mu / ls [B, ldc] -> dict of [B] arrays"""
    nll, la, mu, ls = (np.asarray(v, dtype) for v in (nll, la, mu, ls))
    B, S_, Kd = nll.shape
    K = la.shape[1]
    logK = dtype(math.log(K))
    q = np.exp(la)
    kl_c = dtype(0.5) * (mu * mu + np.exp(dtype(2) * ls) - dtype(2) * ls - dtype(1)).sum(axis=1, dtype=dtype)
    with np.errstate(invalid="ignore"):
        kl_d = np.where(q != 0, q * (la + logK), dtype(0)).sum(axis=1, dtype=dtype)
        if Kd == 1:
            recon = nll[:, :, 0].sum(axis=1, dtype=dtype) / dtype(S_)
            inner = -nll[:, :, 0]
        else:
            recon = np.where(q[:, None, :] != 0, q[:, None, :] * nll, dtype(0)).sum(axis=(1, 2), dtype=dtype) / dtype(S_)
            inner = lse(-nll - logK, 2, dtype)
    out = dict(recon=recon, kl_c=kl_c, kl_d=kl_d, elbo=-(recon + kl_c + kl_d))
    if lw is not None:
        out["log_px"] = lse(np.asarray(lw, dtype) + inner, 1, dtype) - dtype(math.log(S_)) + dtype(add)
    return out
