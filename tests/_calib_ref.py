"""The restatement of csrc/calib.hip and shot_vae_amd/calibration.py in numpy: every definition of include/shotvae_hip.h once more, in
float64 (the reference) or, with dtype=np.float32, in the arithmetic the kernels use (the yardstick of the project's 8x rule: a GPU
result may be 8 x as far from float64 as this is, on the same inputs).  tests/test_calib_cpu.py pins it to scikit-learn, scipy and
hand-counted cases; tests/test_calib_gpu.py compares the kernels with it.  Seeded generators for the cases both files use."""
import math

import numpy as np

LOGIT, PROB = 0, 1               # include/shotvae_hip.h: SV_CAL_*
ROW_FIELDS = ("conf", "nll", "brier", "entropy")


# ================================================================================================ inputs
def logits(N, K, scale, seed, at_argmax=0.7):
    """normal logits of the given scale (fp32 values) and labels, `at_argmax` of them at the row's maximum"""
    rng = np.random.RandomState(seed)
    x = (scale * rng.randn(N, K)).astype(np.float32)
    label = np.where(rng.uniform(size=N) < at_argmax, x.argmax(axis=1), rng.randint(0, K, size=N)).astype(np.int64)
    return x, label


def probabilities(N, K, scale, seed):
    """softmax of such logits, as fp32 probabilities (rows sum to 1 up to rounding)"""
    x, label = logits(N, K, scale, seed)
    e = np.exp(x.astype(np.float64) - x.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32), label


def quarters(n, seed, lo=-2.0, hi=2.0):
    """scores rounded to quarters: many ties"""
    return (np.round(np.random.RandomState(seed).uniform(lo, hi, size=n) * 4.0) / 4.0).astype(np.float32)


def detection_case(seed=901, n_pos=257, n_neg=130):
    """257 positives around +0.5 and 130 negatives around -0.5, rounded to quarters -> (score fp32, positive int64), shuffled"""
    rng = np.random.RandomState(seed)
    score = np.concatenate([0.5 + rng.randn(n_pos), -0.5 + rng.randn(n_neg)])
    score = (np.round(score * 4.0) / 4.0).astype(np.float32)
    positive = np.concatenate([np.ones(n_pos), np.zeros(n_neg)]).astype(np.int64)
    order = rng.permutation(n_pos + n_neg)
    return score[order], positive[order]


# ================================================================================================ sv_calib_rows
def _u(x, kind, dtype):
    x = np.asarray(x).astype(dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(x) if kind == PROB else x


def rows(x, K, label=None, kind=LOGIT, T=1.0, dtype=np.float64):
    """-> dict(pred int64, conf, nll, brier, entropy, gap): sv_calib_rows on the first K columns of x.  gap = the distance of the two
    largest z of a row (inf for K = 1).  dtype float64: the definitions; float32: the kernel's arithmetic (z = u / T in fp32, the
    entropy as log S - sum e (z - m) / S)."""
    x = np.asarray(x)[:, :K]
    N = x.shape[0]
    T = dtype(np.float32(T))
    with np.errstate(all="ignore"):
        z = (_u(x, kind, dtype) / T).astype(dtype)
        bad = np.isnan(z).any(axis=1) | np.isposinf(z).any(axis=1) | np.isneginf(z).all(axis=1) | (not T > 0)
        zs = np.where(bad[:, None], dtype(0), z)
        m = zs.max(axis=1)
        pred = zs.argmax(axis=1).astype(np.int64)                  # the first maximum
        d = (zs - m[:, None]).astype(dtype)
        e = np.exp(d).astype(dtype)
        S = e.sum(axis=1, dtype=dtype)
        logS = np.log(S).astype(dtype)
        p = (e / S[:, None]).astype(dtype)
        if dtype == np.float64:
            logp = d - logS[:, None]
            entropy = -np.where(p > 0, p * np.where(p > 0, logp, 0.0), 0.0).sum(axis=1)
        else:
            entropy = logS - np.where(e > 0, e * np.where(e > 0, d, dtype(0)), dtype(0)).sum(axis=1, dtype=dtype) / S
        conf = (dtype(1) / S).astype(dtype)
        lab = np.full(N, -1, dtype=np.int64) if label is None else np.asarray(label, dtype=np.int64)
        ok = (lab >= 0) & (lab < K)
        at = np.where(ok, lab, 0)
        onehot = (np.arange(K)[None, :] == at[:, None]).astype(dtype)
        nll = logS - d[np.arange(N), at]
        brier = ((p - onehot) ** 2).sum(axis=1, dtype=dtype)
        srt = np.sort(zs, axis=1)
        gap = srt[:, -1] - srt[:, -2] if K > 1 else np.full(N, np.inf)
    nan = dtype(np.nan)
    return dict(pred=np.where(bad, -1, pred), conf=np.where(bad, nan, conf), entropy=np.where(bad, nan, entropy),
                nll=np.where(bad | ~ok, nan, nll), brier=np.where(bad | ~ok, nan, brier), gap=np.where(bad, nan, gap).astype(np.float64))


def row_allowance(x, K, label, kind, T):
    """-> (float64 reference, {field: 8 x the largest error of the fp32 restatement against it over the case's rows})"""
    ref, low = rows(x, K, label, kind, T), rows(x, K, label, kind, T, dtype=np.float32)
    tol = {}
    for f in ROW_FIELDS:
        both = ~np.isnan(ref[f])
        assert np.array_equal(both, ~np.isnan(low[f])), f
        with np.errstate(invalid="ignore"):                    # (inf - inf: a label of probability 0)
            err = np.abs(low[f][both].astype(np.float64) - ref[f][both])
        tol[f] = 8.0 * float(err[np.isfinite(err)].max()) if np.isfinite(err).any() else 0.0
    return ref, tol


# ================================================================================================ sv_calib_accum / sv_calib_finish
def uniform_edges(B):
    return np.linspace(0.0, 1.0, B + 1).astype(np.float32)


def bin_of(conf, edges):
    """b = #{ i in 1 .. B-1 : edges[i] < conf }, compared in fp32"""
    conf, inner = np.asarray(conf, dtype=np.float32), np.asarray(edges, dtype=np.float32)[1:-1]
    return (inner[None, :] < conf[:, None]).sum(axis=1).astype(np.int64)


def accum(conf, pred, label, nll, brier, entropy, K, edges, P, state=None):
    """one call of sv_calib_accum -> (bin_count [B], bin_correct [B], counts [3], sums [P, B + 3]); state: those of an earlier call
    (init = 0), None: init = 1 with zeroed integers.  The sums are added row by row, in index order within a state."""
    B, N = len(edges) - 1, len(conf)
    if state is None:
        state = (np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(3, np.int64), np.zeros((P, B + 3)))
    bc, bk, counts, sums = (a.copy() for a in state)
    valid = (np.asarray(pred) >= 0) & (np.asarray(label) >= 0) & (np.asarray(label) < K)
    b = bin_of(conf, edges)
    for i in np.nonzero(valid)[0]:
        p = (i // 64) % P
        bc[b[i]] += 1
        hit = int(pred[i] == label[i])
        bk[b[i]] += hit
        counts[1] += hit
        sums[p, b[i]] += np.float64(conf[i])
        for slot, arr in enumerate((nll, brier, entropy)):
            if arr is not None:
                sums[p, B + slot] += np.float64(arr[i])
    counts[0] += int(valid.sum())
    counts[2] += N
    return bc, bk, counts, sums


def finish(bin_count, bin_correct, counts, sums):
    """-> (out float64 [8], diagram float64 [2, B]): sv_calib_finish before its one rounding to fp32"""
    B = len(bin_count)
    merged = np.zeros(B + 3)
    for p in range(sums.shape[0]):
        merged = merged + sums[p]
    n = float(counts[0])
    out, diagram = np.full(8, np.nan), np.full((2, B), np.nan)
    out[7] = n
    ece, mce, cs = 0.0, -1.0, 0.0
    for b in range(B):
        cs += merged[b]
        if bin_count[b] > 0:
            a, c = float(bin_correct[b]) / float(bin_count[b]), merged[b] / float(bin_count[b])
            diagram[0, b], diagram[1, b] = a, c
            if n > 0:
                ece += float(bin_count[b]) / n * abs(a - c)
            mce = max(mce, abs(a - c))
    if n > 0:
        out[:7] = (float(counts[1]) / n, cs / n, ece, mce if mce >= 0 else np.nan, merged[B] / n, merged[B + 1] / n, merged[B + 2] / n)
    return out, diagram


# ================================================================================================ sv_temp_accum / sv_temp_update
def temp_terms(x, K, label, kind, beta, dtype=np.float64):
    """-> (a, v, nll, valid) per row at beta (used as (float)beta): p = softmax(beta u), a = E_p[u] - u[label], v = Var_p[u]"""
    x = np.asarray(x)[:, :K]
    N = x.shape[0]
    bf = dtype(np.float32(beta))
    lab = np.asarray(label, dtype=np.int64)
    with np.errstate(all="ignore"):
        u = _u(x, kind, dtype)
        z = (bf * u).astype(dtype)
        bad = np.isnan(z).any(axis=1) | np.isposinf(z).any(axis=1) | np.isneginf(z).all(axis=1)
        valid = ~bad & (lab >= 0) & (lab < K)
        u, z = np.where(valid[:, None], u, dtype(0)), np.where(valid[:, None], z, dtype(0))
        at = np.where(valid, lab, 0)
        m = z.max(axis=1)
        e = np.exp(z - m[:, None]).astype(dtype)
        S = e.sum(axis=1, dtype=dtype)
        mean = (np.where(e > 0, e * np.where(e > 0, u, dtype(0)), dtype(0)).sum(axis=1, dtype=dtype) / S).astype(dtype)
        dev = np.where(e > 0, u - mean[:, None], dtype(0)).astype(dtype)
        v = ((e * dev * dev).sum(axis=1, dtype=dtype) / S).astype(dtype)
        ul = u[np.arange(N), at]
        a = (mean - ul).astype(dtype)
        nll = (np.log(S) - (bf * ul - m)).astype(dtype)
    return a, v, nll, valid


def temp_sums(x, K, label, kind, beta, P, dtype=np.float64):
    """sv_temp_accum with init = 1 -> (sums float64 [P, 3], count int64 [P]): the rows of a state in index order"""
    a, v, nll, valid = temp_terms(x, K, label, kind, beta, dtype)
    sums, count = np.zeros((P, 3)), np.zeros(P, np.int64)
    for i in np.nonzero(valid)[0]:
        p = (i // 64) % P
        sums[p] += (np.float64(a[i]), np.float64(v[i]), np.float64(nll[i]))
        count[p] += 1
    return sums, count


def temp_update(sums, count, beta):
    """sv_temp_update -> (beta_new float64, temp fp32, stats float64 [4] before the rounding to fp32)"""
    A = V = Ls = 0.0
    n = 0
    for p in range(sums.shape[0]):
        A, V, Ls, n = A + sums[p, 0], V + sums[p, 1], Ls + sums[p, 2], n + int(count[p])
    new = beta
    if beta > 0 and V > 0 and math.isfinite(A) and math.isfinite(V):
        new = min(max(beta - A / V, 0.25 * beta), 4.0 * beta)
    with np.errstate(all="ignore"):
        stats = np.array([np.float64(Ls) / np.float64(n), np.float64(A) / np.float64(n), new - beta, new])
    return new, np.float32(1.0 / new), stats


def newton(x, K, label, kind=LOGIT, iters=12, dtype=np.float64, beta=1.0, P=1):
    """`iters` iterations of accum + update from beta -> beta"""
    for _ in range(iters):
        beta = temp_update(*temp_sums(x, K, label, kind, beta, P, dtype), beta)[0]
    return beta


def total_nll(x, K, label, kind, beta):
    """the summed NLL at beta, in float64 with beta NOT rounded to fp32 (the function scipy minimises)"""
    u = _u(np.asarray(x)[:, :K], kind, np.float64)
    z = beta * u
    m = z.max(axis=1)
    return float((np.log(np.exp(z - m[:, None]).sum(axis=1)) + m - z[np.arange(len(z)), np.asarray(label)]).sum())


# ================================================================================================ sv_rank_scan and what is built on it
def rank_counts(q, g, w=None):
    """-> (greater, equal) int64 [Q]: IEEE comparisons of the fp32 values, weights int64 (None: 1)"""
    q, g = np.asarray(q, dtype=np.float32), np.asarray(g, dtype=np.float32)
    w = np.ones(len(g), np.int64) if w is None else np.asarray(w, dtype=np.int64)
    gt, eq = np.zeros(len(q), np.int64), np.zeros(len(q), np.int64)
    with np.errstate(invalid="ignore"):
        for i0 in range(0, len(q), 512):
            qq = q[i0:i0 + 512, None]
            gt[i0:i0 + 512] = np.where(g[None, :] > qq, w[None, :], 0).sum(axis=1)
            eq[i0:i0 + 512] = np.where(g[None, :] == qq, w[None, :], 0).sum(axis=1)
    return gt, eq


def detection(score, positive, tpr=0.95):
    """-> dict(auroc, aupr, aupr_neg, fpr_at_tpr): the count formulas of shot_vae_amd.calibration.detection_metrics in float64"""
    score = np.asarray(score, dtype=np.float32)
    seen = ~np.isnan(score)
    pos, neg = (np.asarray(positive) != 0) & seen, (np.asarray(positive) == 0) & seen
    gp, ep = rank_counts(score, score, pos.astype(np.int64))
    gn, en = rank_counts(score, score, neg.astype(np.int64))
    n_pos, n_neg = int(pos.sum()), int(neg.sum())
    with np.errstate(all="ignore"):
        tp, fp = (gp + ep).astype(np.float64), (gn + en).astype(np.float64)
        auroc = np.float64((n_neg - gn[pos] - 0.5 * en[pos]).sum()) / np.float64(n_pos * n_neg)
        aupr = np.float64((tp[pos] / (tp[pos] + fp[pos])).sum()) / np.float64(n_pos)
        tn_le, fn_le = (n_neg - gn).astype(np.float64), (n_pos - gp).astype(np.float64)
        aupr_neg = np.float64((tn_le[neg] / (tn_le[neg] + fn_le[neg])).sum()) / np.float64(n_neg)
        reach = pos & (tp / np.float64(n_pos) >= tpr)
        fpr = float((fp[reach] / np.float64(n_neg)).min()) if reach.any() and n_neg else float("nan")
    return dict(auroc=float(auroc), aupr=float(aupr), aupr_neg=float(aupr_neg), fpr_at_tpr=fpr)


def selective(conf, correct):
    """-> dict(aurc, e_aurc): tied rows share their group's risk"""
    conf = np.asarray(conf, dtype=np.float32)
    wrong = (np.asarray(correct) == 0).astype(np.int64)
    g, e = rank_counts(conf, conf)
    gw, ew = rank_counts(conf, conf, wrong)
    n, errors = len(conf), int(wrong.sum())
    with np.errstate(all="ignore"):
        aurc = float(((gw + ew) / (g + e).astype(np.float64)).mean())
    best = sum((i - (n - errors)) / i for i in range(n - errors + 1, n + 1)) / n
    return dict(aurc=aurc, e_aurc=aurc - best)
