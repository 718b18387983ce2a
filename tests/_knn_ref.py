"""numpy restatement of csrc/knn.hip's definitions (include/shotvae_hip.h), float64 unless a dtype is given: the four metrics in the
direct-difference form, the stable top-k with the index tie rule, both votes and the counters.  tests/test_knn_cpu.py pins it to the
reference's own outputs (tests/golden/ref_calculate_dist.npz); the GPU tests measure their allowances with it."""
import numpy as np

METRICS = ("kl", "w2", "euclid", "cosine")
CODE = {"kl": 0, "w2": 1, "euclid": 2, "cosine": 3}


def distances(metric, mu1, ls1, mu2, ls2, dtype=np.float64):
    """[n1, n2] in `dtype`, every operation carried out in it: sums over the differences themselves, query (first argument) first"""
    mu1, mu2 = np.asarray(mu1, dtype=dtype), np.asarray(mu2, dtype=dtype)
    dm = mu1[:, None, :] - mu2[None, :, :]
    if metric == "euclid":
        return np.sum(dm * dm, axis=2)
    if metric == "cosine":
        n1, n2 = np.sum(mu1 * mu1, axis=1), np.sum(mu2 * mu2, axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.sum(mu1[:, None, :] * mu2[None, :, :], axis=2) / (n1[:, None] * n2[None, :])
    ls1, ls2 = np.asarray(ls1, dtype=dtype), np.asarray(ls2, dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        if metric == "w2":
            ds = np.exp(ls1)[:, None, :] - np.exp(ls2)[None, :, :]
            return np.sum(dm * dm, axis=2) + np.sum(ds * ds, axis=2)
        if metric == "kl":
            v1, iv2 = np.exp(dtype(2) * ls1), np.exp(dtype(-2) * ls2)
            t = (ls2[None, :, :] - ls1[:, None, :]) + dtype(0.5) * ((v1[:, None, :] + dm * dm) * iv2[None, :, :] - dtype(1))
            return np.sum(t, axis=2)
    raise ValueError(metric)


def topk(dist, k, metric, col0=0, self0=-1):
    """(val [Q, k] float64, idx [Q, k] int64) of the distance matrix `dist` [Q, N] whose column r is global index col0 + r: the k
    closest per row, closest first (largest first for the cosine), equal values by the smaller index.  A NaN, a distance of +inf (a
    similarity of -inf) and global index self0 + i for row i (self0 >= 0) never enter; empty slots are idx -1, val +inf (-inf)."""
    dist = np.asarray(dist, dtype=np.float64)
    Q, N = dist.shape
    sign = -1.0 if metric == "cosine" else 1.0
    val = np.full((Q, k), sign * np.inf)
    idx = np.full((Q, k), -1, dtype=np.int64)
    for i in range(Q):
        key = sign * dist[i]
        ok = key < np.inf                                   # False for NaN
        if self0 >= 0 and 0 <= self0 + i - col0 < N:
            ok[self0 + i - col0] = False
        cols = np.nonzero(ok)[0]
        order = cols[np.argsort(key[cols], kind="stable")][:k]          # stable: ties keep the index order
        val[i, :len(order)] = dist[i, order]
        idx[i, :len(order)] = order + col0
    return val, idx


def vote(val, idx, g_label, K, mode=0, tau=1.0):
    """(votes [Q, K] float64, pred [Q] int64): a slot votes when its index is in the gallery and its label in [0, K); weight 1 (mode 0),
    exp(-val / tau) (1), exp(val / tau) (2); pred = the first maximum, -1 when no slot voted"""
    g_label = np.asarray(g_label)
    Q, k = idx.shape
    votes = np.zeros((Q, K))
    pred = np.full(Q, -1, dtype=np.int64)
    for i in range(Q):
        n = 0
        for s in range(k):
            g = idx[i, s]
            if 0 <= g < len(g_label) and 0 <= g_label[g] < K:
                w = 1.0 if mode == 0 else np.exp((-val[i, s] if mode == 1 else val[i, s]) / tau)
                votes[i, g_label[g]] += w
                n += 1
        if n:
            pred[i] = int(np.argmax(votes[i]))
    return votes, pred


def counters(pred, q_label, K):
    """(counts [2], confusion [K, K]) int64 of one call: hits and rows; a label outside [0, K) or a pred of -1 is a row only"""
    counts = np.array([int(np.sum((pred >= 0) & (pred == q_label))), len(pred)], dtype=np.int64)
    conf = np.zeros((K, K), dtype=np.int64)
    for p, y in zip(pred, q_label):
        if p >= 0 and 0 <= y < K:
            conf[y, p] += 1
    return counts, conf


def posterior(n, d, stream):
    """the inputs of the GPU tests: mu ~ N(0, 1), log sigma ~ U(-1, 0.5) (closed forms), fp32 values as float64 arrays"""
    from tests.golden import make_dist_goldens as G
    return G.posterior(n, d, stream)


def tolerance(metric, mu1, ls1, mu2, ls2, ref=None):
    """the 8x rule: 8 x the largest error of the fp32 restatement against the float64 one on these inputs (absolute)"""
    ref = distances(metric, mu1, ls1, mu2, ls2) if ref is None else ref
    f32 = distances(metric, mu1, ls1, mu2, ls2, dtype=np.float32).astype(np.float64)
    fin = np.isfinite(ref) & np.isfinite(f32)
    return 8.0 * float(np.max(np.abs(f32 - ref)[fin]))


_TOL = {}


def tolerance_for(metric, D):
    """the 8x rule for rows of `D` dimensions: measured once per (metric, D) on 64 x 64 pairs of posterior() rows, so that a case of a
    few pairs is not judged by the luck of its own handful of roundings"""
    if (metric, D) not in _TOL:
        mu1, ls1 = posterior(64, D, 9990)
        mu2, ls2 = posterior(64, D, 9992)
        _TOL[metric, D] = tolerance(metric, mu1, ls1, mu2, ls2)
    return _TOL[metric, D]


def vote32(val, idx, g_label, K, mode, tau):
    """votes of vote() with every weight and sum in fp32, slot order: the fp32 restatement the weighted votes' 8x rule is measured from"""
    g_label = np.asarray(g_label)
    votes = np.zeros((idx.shape[0], K), dtype=np.float32)
    for i in range(idx.shape[0]):
        for s in range(idx.shape[1]):
            g = idx[i, s]
            if 0 <= g < len(g_label) and 0 <= g_label[g] < K:
                v = np.float32(val[i, s])
                votes[i, g_label[g]] += np.exp((-v if mode == 1 else v) / np.float32(tau), dtype=np.float32)
    return votes


# ---- the evaluate_knn cases: closed-form models and images (oracle/closed_form.py), gallery 96 images, test set 48, batches of 16 ----
EVAL_K, EVAL_B, EVAL_GALLERY, EVAL_TEST, EVAL_CLASSES = 5, 16, 96, 48, 10
EVAL_KINDS = ("wideresnet-10-1", "svhn")
# (model, metric) of the evaluate_knn cases.  "kl" is not among them: the posteriors of a closed-form (untrained) encoder nearly
# coincide -- KL values of 4e-5 .. 2e-3 against an fp32 error of 1e-5 from the -1 in every term -- so that NO row's 5th and 6th
# neighbour are 4 tolerances apart (48 of 48 undecided for both models, measured with the CPU oracle); the differences of "euclid"
# and "w2" carry no such constant and leave 0 rows undecided.
EVAL_CASES = (("wideresnet-10-1", "euclid"), ("svhn", "w2"), ("svhn", "euclid"))
MAX_UNDECIDED = EVAL_TEST // 10


def eval_images(kind):
    """(gallery images, gallery labels, test images, test labels), CPU tensors"""
    import torch
    from oracle import closed_form as C
    g = C.uniform((EVAL_GALLERY, 3, 32, 32), 9950)
    t = C.uniform((EVAL_TEST, 3, 32, 32), 9951)
    return g, (torch.arange(EVAL_GALLERY) * 7 + 3) % EVAL_CLASSES, t, (torch.arange(EVAL_TEST) * 3 + 1) % EVAL_CLASSES


def eval_state(kind):
    from oracle import closed_form as C
    from oracle import smooth_oracle as SO
    return SO.make_state("svhn") if kind == "svhn" else C.make_state(kind, K=EVAL_CLASSES)


def eval_oracle_posterior(kind, x):
    """(mu, log sigma) float64 numpy of the CPU oracle in eval mode -- only to choose the inputs: the GPU test feeds the restatement
    with the model's OWN encode outputs"""
    import torch
    from oracle import shotvae_oracle as O
    from oracle import smooth_oracle as SO
    st = eval_state(kind)
    with torch.no_grad():
        if kind == "svhn":
            _, mean, logvar, _, _ = SO.forward(st, kind, x, torch.zeros(x.shape[0], 32), training=False)
            return mean.double().numpy(), 0.5 * logvar.double().numpy()
        _, mu, ls, _ = O.vae_forward(st, kind, x, torch.zeros(x.shape[0], 128), label=torch.zeros(x.shape[0], dtype=torch.int64),
                                     training=False, update=False)
        return mu.double().numpy(), ls.double().numpy()


def decided_rows(metric, mu_q, ls_q, mu_g, ls_g, k):
    """(decided bool [Q], tol, ref distances): a row is decided when the float64 gap between its k-th and (k+1)-th neighbour exceeds
    4 x the 8x-rule tolerance measured on these inputs -- no fp32 rounding can then change the set of its k neighbours"""
    ref = distances(metric, mu_q, ls_q, mu_g, ls_g)
    tol = tolerance(metric, mu_q, ls_q, mu_g, ls_g, ref)
    key = np.sort(-ref if metric == "cosine" else ref, axis=1)
    return (key[:, k] - key[:, k - 1]) > 4.0 * tol, tol, ref
