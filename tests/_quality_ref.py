"""float64 numpy restatement of csrc/manifold.hip's definitions (include/shotvae_hip.h: sv_ball_scan) and of shot_vae_amd/quality.py: the
k-th-neighbour radii (tests/_knn_ref.topk, leave-one-out), the membership counts with their rules, precision / recall / density /
coverage, the shifted-data moments and the symmetric Frechet formula.  tests/test_quality_cpu.py pins it to closed forms, numpy.cov and
(where it is installed) scipy.linalg.sqrtm; the GPU tests compare the kernels and the Python layer with it."""
import numpy as np

from tests import _knn_ref as R


def radii(metric, mu, ls, k):
    """[n] float64: the distance of every row to its k-th nearest OTHER row of the set"""
    dist = R.distances(metric, mu, ls, mu, ls)
    return R.topk(dist, k, metric, col0=0, self0=0)[0][:, k - 1]


def inside(dist, r, col0=0, self0=-1):
    """bool [Q, N]: the value is finite, <= the column's radius, and the column (global index col0 + j) is not self0 + i.  A NaN value or
    radius contains nothing, +inf every finite value, a negative radius nothing, 0 the coincident rows"""
    dist, r = np.asarray(dist, dtype=np.float64), np.asarray(r, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        m = np.isfinite(dist) & (dist <= r[None, :])
    if self0 >= 0:
        for i in range(dist.shape[0]):
            j = self0 + i - col0
            if 0 <= j < dist.shape[1]:
                m[i, j] = False
    return m


def counts(dist, r, col0=0, self0=-1):
    """(q_count [Q], g_count [N]) int64"""
    m = inside(dist, r, col0, self0)
    return m.sum(axis=1).astype(np.int64), m.sum(axis=0).astype(np.int64)


def metrics(metric, real_mu, real_ls, fake_mu, fake_ls, k):
    """manifold_metrics' dict: balls to the k-th neighbour within each set; fake rows against real balls, real rows against fake balls"""
    n_real, n_fake = len(real_mu), len(fake_mu)
    in_real, held = counts(R.distances(metric, fake_mu, fake_ls, real_mu, real_ls), radii(metric, real_mu, real_ls, k))
    in_fake, _ = counts(R.distances(metric, real_mu, real_ls, fake_mu, fake_ls), radii(metric, fake_mu, fake_ls, k))
    return dict(precision=float((in_real > 0).sum()) / n_fake, recall=float((in_fake > 0).sum()) / n_real,
                density=float(in_real.sum()) / (k * n_fake), coverage=float((held > 0).sum()) / n_real, n_real=n_real, n_fake=n_fake)


def moments(x):
    """(mean [D], unbiased covariance [D, D]) of the rows x, two passes in float64"""
    x = np.asarray(x, dtype=np.float64)
    m = x.mean(axis=0)
    c = x - m
    return m, c.T @ c / (x.shape[0] - 1)


def shifted_moments(batches):
    """FeatureMoments' arithmetic: n, sum (x - shift), sum (x - shift)(x - shift)^T with shift = the first batch's mean -> (mean, cov)"""
    shift = n = s1 = s2 = None
    for x in batches:
        x = np.asarray(x, dtype=np.float64)
        if shift is None:
            shift, n, s1, s2 = x.mean(axis=0), 0.0, np.zeros(x.shape[1]), np.zeros((x.shape[1], x.shape[1]))
        c = x - shift
        n, s1, s2 = n + x.shape[0], s1 + c.sum(axis=0), s2 + c.T @ c
    return shift + s1 / n, (s2 - np.outer(s1, s1) / n) / (n - 1.0)


def moment_terms(x, shift):
    """(sum |x - shift| [D], sum |x - shift| |x - shift|^T [D, D]): the absolute terms the sums over the n rows add up -- a sum of n
    terms in any order is within n 2^-53 sum |terms| of the exact one"""
    c = np.abs(np.asarray(x, dtype=np.float64) - shift)
    return c.sum(axis=0), c.T @ c


def psd_spectrum(w):
    """negative eigenvalues, and those within len(w) eps of the largest (eigh's own error), are zero"""
    top = max(float(np.max(w)), 0.0)
    return np.where(w > len(w) * np.finfo(np.float64).eps * top, w, 0.0)


def frechet(m1, s1, m2, s2):
    """|m1 - m2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1^1/2 S2 S1^1/2): the symmetric form, real arithmetic only"""
    m1, s1, m2, s2 = (np.asarray(a, dtype=np.float64) for a in (m1, s1, m2, s2))
    w, v = np.linalg.eigh(s1)
    h = v @ np.diag(np.sqrt(psd_spectrum(w))) @ v.T
    mid = h @ s2 @ h
    ev = psd_spectrum(np.linalg.eigvalsh((mid + mid.T) / 2.0))
    return float(np.sum((m1 - m2) ** 2) + np.trace(s1) + np.trace(s2) - 2.0 * np.sum(np.sqrt(ev)))


def frechet_of_rows(a, b):
    return frechet(*moments(a), *moments(b))
