"""Are two sets of rows drawn from one distribution?  Kernel two-sample statistics on the HIP path (csrc/ksum.hip): the
maximum mean discrepancy (Gretton et al. 2012) with its witness function and permutation test, and the kernel inception distance
(Binkowski et al. 2018) -- the unbiased polynomial-kernel MMD^2 over random subsets.

    kernel_sums(x, y)                                   # double [n]: sum_j k(x_i, y_j), RBF at the median bandwidth
    mmd2(x, y)                                          # the unbiased MMD^2, a float64 device scalar
    witness(x, y, at)                                   # mean_j k(at_i, x_j) - mean_j k(at_i, y_j): which rows carry the difference
    permutation_test(x, y, permutations=200)            # statistic, p_value
    kid(real, fake)                                     # kid_mean, kid_std (torch-fidelity's defaults)

    evaluate_two_sample(model, loader_a, loader_b)      # the codes of two image sets: shift between train and test, ...
    evaluate_prior_match(model, loader)                 # sampled codes z ~ q(z | x) against the N(0, I) prior (the WAE / InfoVAE term)
    evaluate_kid(model, loader)                         # the model's own samples against the images

Kernels: "rbf" k = sum_s w_s exp(-a_s |x - y|^2), "imq" k = sum_s w_s / (1 + a_s |x - y|^2) (the WAE kernel), "poly" k = (a x.y + c)^degree.
The [n, m] kernel matrix is never stored; every sum is taken in double in a fixed order (the same bits on every run); nothing here
synchronises with the host except where stated, and there is no CPU fallback."""
import torch

from . import _lib as L
from ._latent import _p, _st, eval_only, gather_codes, latent_family, matrix, on_device, regroup
from .aggregate import AggregatePosterior, partials
from .neighbors import encode_posterior, pairwise_distance

KINDS = {"rbf": L.KSUM_RBF, "imq": L.KSUM_IMQ, "poly": L.KSUM_POLY}
MAX_SCALES, MAX_DEGREE, MAX_PROBLEMS = 8, 8, 65535


# ---- the kernel's parameters: a device array double [n_scale][2] ----
def _kind(what, kernel):
    if kernel not in KINDS:
        raise ValueError("%s: unknown kernel %r (one of 'rbf', 'imq', 'poly')" % (what, kernel))
    return KINDS[kernel]


def _degree(what, degree):
    if isinstance(degree, bool) or int(degree) != degree or not 1 <= int(degree) <= MAX_DEGREE:
        raise ValueError("%s: degree must be an integer in [1, %d]" % (what, MAX_DEGREE))
    return int(degree)


def _check_gamma(what, kernel, gamma, scales):
    """what needs no device: the form of gamma and scales"""
    if scales is not None:
        if isinstance(gamma, str) and gamma != "median" or not isinstance(gamma, str) and (
                torch.is_tensor(gamma) and gamma.numel() != 1 or isinstance(gamma, (list, tuple))):
            raise ValueError("%s: scales multiply ONE bandwidth ('median', a number or a 1-element tensor)" % what)
        if not isinstance(scales, (list, tuple)) or not 1 <= len(scales) <= MAX_SCALES or any(not float(c) > 0.0 for c in scales):
            raise ValueError("%s: scales must be 1 .. %d positive numbers" % (what, MAX_SCALES))
    if isinstance(gamma, str):
        if gamma != "median":
            raise ValueError("%s: gamma must be 'median', a number, a sequence of numbers or a device tensor" % what)
        if kernel == "poly":
            raise ValueError("%s: the median bandwidth belongs to 'rbf' and 'imq'; 'poly' takes a number (None: 1 / D)" % what)
    elif gamma is None:
        if kernel != "poly":
            raise ValueError("%s: gamma=None (1 / D) belongs to 'poly'" % what)
    elif torch.is_tensor(gamma):
        if gamma.numel() < 1 or gamma.dim() > 2 or (gamma.dim() == 2 and gamma.shape[1] != 2) or not gamma.dtype.is_floating_point:
            raise ValueError("%s: a gamma tensor is a scalar, a vector of bandwidths or a parameter array [n_scale, 2]" % what)
        n = gamma.shape[0] if gamma.dim() == 2 else gamma.numel()
        if n > (1 if kernel == "poly" else MAX_SCALES):
            raise ValueError("%s: %d scales, at most %d" % (what, n, 1 if kernel == "poly" else MAX_SCALES))
    elif isinstance(gamma, (list, tuple)):
        if not 1 <= len(gamma) <= (1 if kernel == "poly" else MAX_SCALES):
            raise ValueError("%s: gamma must hold 1 .. %d bandwidths" % (what, 1 if kernel == "poly" else MAX_SCALES))
        [float(a) for a in gamma]
    else:
        float(gamma)


def kernel_params(kernel, gamma, dim, device, coef0=1.0, scales=None, pool=None, what="kernel_params"):
    """-> the parameter array of sv_ksum_scan, float64 [n_scale, 2] on `device`, built without a host read.  'rbf' / 'imq': rows (a_s,
    w_s) with equal weights 1 / n_scale -- gamma a number, a sequence, a device tensor (a scalar, a vector of bandwidths, or the array
    itself [n_scale, 2]) or "median" (median_bandwidth of the rows `pool` = (x, y)); scales=(c, ..) turns one bandwidth a into the ladder
    a c.  'poly': the one row (gamma, coef0), gamma None = 1 / dim."""
    _kind(what, kernel)
    _check_gamma(what, kernel, gamma, scales)
    on_device(what, gamma)
    if kernel == "poly":
        if torch.is_tensor(gamma):
            if gamma.dim() == 2:
                return gamma.detach().to(device=device, dtype=torch.float64).contiguous()
            a = gamma.detach().to(device=device, dtype=torch.float64).reshape(1)
        else:
            a = torch.tensor([1.0 / dim if gamma is None else float(gamma)], dtype=torch.float64, device=device)
        return torch.stack([a, torch.full_like(a, float(coef0))], dim=1).contiguous()
    if isinstance(gamma, str):
        a = median_bandwidth(*pool).reshape(1)
    elif torch.is_tensor(gamma):
        if gamma.dim() == 2:
            return gamma.detach().to(device=device, dtype=torch.float64).contiguous()
        a = gamma.detach().to(device=device, dtype=torch.float64).reshape(-1)
    else:
        a = torch.tensor([float(v) for v in (gamma if isinstance(gamma, (list, tuple)) else [gamma])], dtype=torch.float64, device=device)
    if scales is not None:
        a = a * torch.tensor([float(c) for c in scales], dtype=torch.float64, device=device)
    return torch.stack([a, torch.full_like(a, 1.0 / a.numel())], dim=1).contiguous()


def median_bandwidth(x, y=None, max_rows=2048, seed=0, scales=None):
    """The median heuristic on the device: a = 1 / median of the squared distances (pairwise_distance(.., "euclid")) between the pooled
    rows of x and y -- all of them, or a subsample of max_rows rows (torch.randperm under a CPU generator seeded with `seed`, its first
    max_rows entries).  The median is the LOWER one of the off-diagonal entries (kthvalue: an element of the matrix, never a mean of
    two).  -> a float64 device scalar; with scales=(c, ..) the ladder a c, float64 [len(scales)].  No host read."""
    _pair("median_bandwidth", x, x if y is None else y)
    max_rows, pooled = int(max_rows), x.shape[0] + (0 if y is None else y.shape[0])
    if max_rows < 2 or pooled < 2:
        raise ValueError("median_bandwidth: a distance needs two rows (max_rows=%d, %d pooled rows)" % (max_rows, pooled))
    if scales is not None:
        _check_gamma("median_bandwidth", "rbf", "median", scales)
    x = matrix("median_bandwidth", x)
    rows = x if y is None else torch.cat([x, matrix("median_bandwidth", y)])
    if rows.shape[0] > max_rows:
        pick = torch.randperm(rows.shape[0], generator=torch.Generator().manual_seed(int(seed)))[:max_rows]
        rows = rows[pick.to(rows.device)]
    n = rows.shape[0]
    d = pairwise_distance(rows, None, rows, None, "euclid")
    d.fill_diagonal_(float("inf"))                      # the n diagonal entries sort last: the first n (n - 1) are the others
    med = torch.kthvalue(d.reshape(-1), (n * (n - 1) + 1) // 2).values.double()
    a = 1.0 / med
    return a if scales is None else a * torch.tensor([float(c) for c in scales], dtype=torch.float64, device=a.device)


# ---- the scan ----
def _scan(what, kind, kparam, degree, q, g, g_w=None, self_from=-1, total=False, q_w=None):
    """sv_ksum_scan + sv_ksum_finish over S problems: q [Q, D] or [S, Q, D], g [N, D] or [S, N, D], g_w None, [N] or [S, N] (fp32,
    contiguous, on the device; a 2-d q or g and a 1-d g_w are shared by the problems) -> (row_sum double [S, Q], total double [S] or
    None); q_w (as g_w, against Q) weights the total"""
    S = max(q.shape[0] if q.dim() == 3 else 1, g.shape[0] if g.dim() == 3 else 1, g_w.shape[0] if g_w is not None and g_w.dim() == 2 else 1)
    Q, D, N = q.shape[-2], q.shape[-1], g.shape[-2]
    if S > MAX_PROBLEMS:
        raise ValueError("%s: %d problems in one launch, at most %d" % (what, S, MAX_PROBLEMS))
    P = partials(-(-Q // 64) * S, N)
    part = torch.empty(S, P, Q, dtype=torch.float64, device=q.device)
    rows = torch.empty(S, Q, dtype=torch.float64, device=q.device)
    tot = torch.empty(S, dtype=torch.float64, device=q.device) if total else None
    L.call("sv_ksum_scan", kind, _p(kparam), kparam.shape[0], degree, _p(q), Q, Q * D if q.dim() == 3 else 0, _p(g), _p(g_w), N,
           N * D if g.dim() == 3 else 0, N if g_w is not None and g_w.dim() == 2 else 0, D, S, 0, self_from, P, _p(part), _st())
    L.call("sv_ksum_finish", _p(part), S, P, Q, 0, _p(rows), _p(q_w) if total else None,
           Q if q_w is not None and q_w.dim() == 2 else 0, _p(tot), _st())
    return rows, tot


def _weights(what, weights, n):
    if weights is None:
        return None
    if not torch.is_tensor(weights) or tuple(weights.shape) != (n,) or not weights.dtype.is_floating_point:
        raise ValueError("%s: weights must be a floating-point vector [%d]" % (what, n))
    on_device(what, weights)
    return weights.detach().float().contiguous()


def _self_from(what, exclude_self_from):
    self_from = -1 if exclude_self_from is None else int(exclude_self_from)
    if self_from < -1:
        raise ValueError("%s: exclude_self_from must be >= 0" % what)
    return self_from


def _pair(what, x, y):
    """shape, then the no-CPU rule, of two row sets of one width"""
    for name, t in (("x", x), ("y", y)):
        if not torch.is_tensor(t) or t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError("%s: %s must be a non-empty matrix [n, d]" % (what, name))
    if x.shape[1] != y.shape[1]:
        raise ValueError("%s: x has %d columns, y %d" % (what, x.shape[1], y.shape[1]))


def kernel_sums(x, y, kernel="rbf", gamma="median", degree=3, coef0=1.0, weights=None, exclude_self_from=None, total=False, scales=None):
    """-> float64 [n]: sum_j w_j k(x_i, y_j) over the rows of y (weights: fp32 [m], None = 1); total=True: -> (the sums, their sum: a
    float64 device scalar).  exclude_self_from = s: x_i is row s + i of y and its own pair is left out.  gamma, scales: kernel_params'
    ("median": the bandwidth of the pooled rows of x and y).  Capturable once the buffers exist: no host read."""
    what = "kernel_sums"
    _pair(what, x, y)
    kind = _kind(what, kernel)
    degree = _degree(what, degree)
    _check_gamma(what, kernel, gamma, scales)
    self_from = _self_from(what, exclude_self_from)
    if weights is not None and (not torch.is_tensor(weights) or tuple(weights.shape) != (y.shape[0],)):
        raise ValueError("%s: weights must be a floating-point vector [%d]" % (what, y.shape[0]))
    x, y = matrix(what, x), matrix(what, y)
    w = _weights(what, weights, y.shape[0])
    kparam = kernel_params(kernel, gamma, x.shape[1], x.device, coef0, scales, (x, y), what)
    rows, tot = _scan(what, kind, kparam, degree, x, y, w, self_from, total)
    return (rows[0], tot[0]) if total else rows[0]


def _mmd2_of(kind, kparam, degree, x, y, unbiased):
    """the statistic from three scans; x [n, D] / [S, n, D], y likewise -> float64 [S]"""
    n, m = x.shape[-2], y.shape[-2]
    sxx = _scan("mmd2", kind, kparam, degree, x, x, None, 0 if unbiased else -1, True)[1]
    syy = _scan("mmd2", kind, kparam, degree, y, y, None, 0 if unbiased else -1, True)[1]
    sxy = _scan("mmd2", kind, kparam, degree, x, y, None, -1, True)[1]
    if unbiased:
        return sxx / (n * (n - 1)) + syy / (m * (m - 1)) - 2.0 * sxy / (n * m)
    return sxx / (n * n) + syy / (m * m) - 2.0 * sxy / (n * m)


def mmd2(x, y, kernel="rbf", gamma="median", degree=3, coef0=1.0, unbiased=True, scales=None):
    """The squared maximum mean discrepancy of the rows x [n, D] and y [m, D], a float64 device scalar (no host read).  unbiased: the
    U-statistic S_xx / (n (n - 1)) + S_yy / (m (m - 1)) - 2 S_xy / (n m) with the self pairs left out (needs n, m >= 2; may be
    negative); otherwise the V-statistic with the diagonal, >= 0 up to rounding.  Three scans; the combination is a cold one in torch."""
    what = "mmd2"
    _pair(what, x, y)
    kind = _kind(what, kernel)
    degree = _degree(what, degree)
    _check_gamma(what, kernel, gamma, scales)
    if unbiased and min(x.shape[0], y.shape[0]) < 2:
        raise ValueError("mmd2: the unbiased statistic needs two rows on each side")
    x, y = matrix(what, x), matrix(what, y)
    kparam = kernel_params(kernel, gamma, x.shape[1], x.device, coef0, scales, (x, y), what)
    return _mmd2_of(kind, kparam, degree, x, y, bool(unbiased))[0]


def witness(x, y, at, kernel="rbf", gamma="median", degree=3, coef0=1.0, scales=None):
    """The empirical witness function of the MMD at the rows `at` [q, D]: mean_j k(at_i, x_j) - mean_j k(at_i, y_j), float64 [q] --
    positive where x has more mass than y.  Two scans, no host read ("median": the bandwidth of x and y, not of `at`)."""
    what = "witness"
    _pair(what, x, y)
    _pair(what, x, at)
    kind = _kind(what, kernel)
    degree = _degree(what, degree)
    _check_gamma(what, kernel, gamma, scales)
    x, y, at = matrix(what, x), matrix(what, y), matrix(what, at)
    kparam = kernel_params(kernel, gamma, x.shape[1], x.device, coef0, scales, (x, y), what)
    sx = _scan(what, kind, kparam, degree, at, x)[0][0]
    sy = _scan(what, kind, kparam, degree, at, y)[0][0]
    return sx / x.shape[0] - sy / y.shape[0]


def subset_indices(n, m, subsets, subset_size, seed):
    """the index sets of kid(): for each subset in turn, the first subset_size entries of torch.randperm(n) and then of
    torch.randperm(m), under ONE CPU generator seeded with `seed` -> (int64 [subsets, size], int64 [subsets, size]), CPU"""
    gen = torch.Generator().manual_seed(int(seed))
    a, b = [], []
    for _ in range(subsets):
        a.append(torch.randperm(n, generator=gen)[:subset_size])
        b.append(torch.randperm(m, generator=gen)[:subset_size])
    return torch.stack(a), torch.stack(b)


def _kid_stats(what, real, fake, subsets, subset_size, degree, gamma, coef0, seed):
    """-> (float64 [2] on the device: mean and population standard deviation of the per-subset MMD^2, the size used, the index sets)"""
    _pair(what, real, fake)
    degree = _degree(what, degree)
    _check_gamma(what, "poly", gamma, None)
    subsets, subset_size = int(subsets), int(subset_size)
    if not 1 <= subsets <= MAX_PROBLEMS:
        raise ValueError("%s: subsets must be in [1, %d]" % (what, MAX_PROBLEMS))
    size = min(subset_size, real.shape[0], fake.shape[0])
    if size < 2:
        raise ValueError("%s: the unbiased MMD^2 of a subset needs two rows on each side (subset_size=%d, %d and %d rows)"
                         % (what, subset_size, real.shape[0], fake.shape[0]))
    real, fake = matrix(what, real), matrix(what, fake)
    kparam = kernel_params("poly", gamma, real.shape[1], real.device, coef0, None, None, what)
    ia, ib = (t.to(real.device) for t in subset_indices(real.shape[0], fake.shape[0], subsets, size, seed))
    xs, ys = real[ia].contiguous(), fake[ib].contiguous()          # one gather per side: [subsets, size, D]
    vals = _mmd2_of(L.KSUM_POLY, kparam, degree, xs, ys, True)
    return torch.stack([vals.mean(), vals.std(unbiased=False)]), size, (ia, ib), vals


def kid(real, fake, subsets=100, subset_size=1000, degree=3, gamma=None, coef0=1.0, seed=0, return_indices=False):
    """The kernel inception distance of the rows fake [m, D] against real [n, D]: the unbiased MMD^2 under the polynomial kernel
    (x.y gamma + coef0)^degree (gamma None: 1 / D) over `subsets` random subsets of subset_size rows of each side, drawn without
    replacement within a subset (subset_indices); torch-fidelity's defaults.  A side with fewer rows than subset_size lowers the size
    to min(n, m), and the result says so.  Three batched scans -- one launch each for all subsets.  -> kid_mean, kid_std (the
    population standard deviation over the subsets), subsets, subset_size (the size used), clipped; return_indices: also `indices`, the
    two index sets on the device, and `values`, the per-subset MMD^2 (float64 on the device).  One host read."""
    stats, size, idx, vals = _kid_stats("kid", real, fake, subsets, subset_size, degree, gamma, coef0, seed)
    mean, std = (float(v) for v in stats.cpu().numpy())
    res = dict(kid_mean=mean, kid_std=std, subsets=int(subsets), subset_size=size, clipped=size < int(subset_size))
    if return_indices:
        res.update(indices=idx, values=vals)
    return res


def split_weights(member, n, m):
    """the weight vectors of the permutation statistic: +m for a row of the first group, -n for a row of the second (the +1 / n and
    -1 / m of the V-statistic times n m: exact in fp32) -> fp32 [S, n + m]"""
    return torch.where(member, float(m), -float(n)).float().contiguous()


def _permutation_stats(what, x, y, kernel, gamma, degree, coef0, scales, permutations, seed, signs):
    """-> float64 [1 + permutations] on the device: the V-statistic of the identity split, then of every permuted split"""
    _pair(what, x, y)
    kind = _kind(what, kernel)
    degree = _degree(what, degree)
    _check_gamma(what, kernel, gamma, scales)
    n, m = x.shape[0], y.shape[0]
    T = n + m
    if signs is None:
        permutations = int(permutations)
        if not 1 <= permutations < MAX_PROBLEMS:
            raise ValueError("%s: permutations must be in [1, %d)" % (what, MAX_PROBLEMS))
    else:
        if not torch.is_tensor(signs) or signs.dim() != 2 or signs.shape[1] != T or not 1 <= signs.shape[0] < MAX_PROBLEMS \
                or signs.dtype != torch.bool:
            raise ValueError("%s: signs must be a bool matrix [permutations, %d] (True: the row goes to the first group)" % (what, T))
        on_device(what, signs)
    if max(n, m) >= 1 << 24:
        raise ValueError("%s: a group of 2^24 rows or more has no exact fp32 weight" % what)
    x, y = matrix(what, x), matrix(what, y)
    if signs is None:
        gen = torch.Generator().manual_seed(int(seed))
        member = torch.zeros(permutations, T, dtype=torch.bool)
        for b in range(permutations):
            member[b, torch.randperm(T, generator=gen)[:n]] = True
        signs = member.to(x.device)
    first = torch.arange(T, device=x.device) < n
    w = split_weights(torch.cat([first[None, :], signs]), n, m)
    pooled = torch.cat([x, y])
    kparam = kernel_params(kernel, gamma, x.shape[1], x.device, coef0, scales, (x, y), what)
    tot = _scan(what, kind, kparam, degree, pooled, pooled, w, -1, True, w)[1]
    return tot / (float(n) * float(m)) ** 2


def p_value_of(stats):
    """(1 + #{b : stat_b >= stat_0}) / (1 + permutations) of a host list whose first entry is the observed statistic"""
    return (1 + sum(1 for s in stats[1:] if s >= stats[0])) / len(stats)


def permutation_test(x, y, kernel="rbf", gamma="median", degree=3, coef0=1.0, scales=None, permutations=200, seed=0, signs=None):
    """The permutation test of H0: x and y are drawn from one distribution.  The rows are pooled; a split gives the rows of its first
    group the weight +1 / n and the others -1 / m, and its statistic is the V-statistic sum_ij w_i w_j k(z_i, z_j) -- the biased MMD^2
    of the split; the identity split comes first, then `permutations` random ones (torch.randperm under a CPU generator seeded with
    `seed`; or `signs`, a bool device matrix [permutations, n + m]: True sends the row to the first group).  ONE scan with shared rows
    and 1 + permutations weight vectors, one finish.  -> statistic, p_value = (1 + #{b : stat_b >= stat_0}) / (1 + permutations),
    statistics (float64 numpy [1 + permutations]).  One host read."""
    stats = _permutation_stats("permutation_test", x, y, kernel, gamma, degree, coef0, scales, permutations, seed, signs).cpu().numpy()
    return dict(statistic=float(stats[0]), p_value=p_value_of(stats.tolist()), statistics=stats)


# ---- the prior side of an RBF kernel, analytic ----
def rbf_prior_expectations(x, kparam):
    """With y, y' ~ N(0, I) in D dimensions and k = sum_s w_s exp(-a_s |.|^2), in float64 torch:
    E_y k(x_i, y) = sum_s w_s (1 + 2 a_s)^(-D / 2) exp(-a_s |x_i|^2 / (1 + 2 a_s))  ([n]) and
    E k(y, y') = sum_s w_s (1 + 4 a_s)^(-D / 2)  (a scalar)"""
    D = x.shape[1]
    r2 = (x.double() ** 2).sum(dim=1)
    a, w = kparam[:, 0], kparam[:, 1]
    exy = (w[None, :] * torch.pow(1.0 + 2.0 * a, -0.5 * D)[None, :] * torch.exp(-a[None, :] * r2[:, None] / (1.0 + 2.0 * a)[None, :])).sum(dim=1)
    eyy = (w * torch.pow(1.0 + 4.0 * a, -0.5 * D)).sum()
    return exy, eyy


# ---- evaluators ----
def _space(what, model, space):
    family = latent_family(what, model)
    if space not in ("mu", "features"):
        raise ValueError("%s: space must be 'mu' or 'features'" % what)
    if space == "features" and family != "shot":
        raise ValueError("%s: space='features' needs a VariationalAutoEncoder (a SmoothVAE has no pooled features)" % what)
    return family


def _chunk(what, chunk_rows):
    if chunk_rows is not None and int(chunk_rows) < 1:
        raise ValueError("%s: chunk_rows must be >= 1 or None" % what)
    return None if chunk_rows is None else int(chunk_rows)


def evaluate_two_sample(model, batches_a, batches_b, space="mu", kernel="rbf", gamma="median", degree=3, coef0=1.0, scales=None,
                        unbiased=True, permutations=0, seed=0, chunk_rows=256):
    """Do the images of batches_a and batches_b look alike to `model` (a VariationalAutoEncoder or a SmoothVAE, in eval mode:
    NotImplementedError otherwise)?  Their codes -- the posterior means (space "mu") or the pooled features ("features") of (image,
    label) batches on the device, regrouped to chunk_rows rows before the model sees them, all rows gathered first: the result does not
    depend on the batching -- under mmd2 and, with permutations > 0, permutation_test (same kernel; "median" is the bandwidth of the
    two code sets).  -> mmd2, n_a, n_b, and with permutations: statistic, p_value.  One host read."""
    what = "evaluate_two_sample"
    _space(what, model, space)
    _kind(what, kernel)
    degree = _degree(what, degree)
    _check_gamma(what, kernel, gamma, scales)
    permutations = int(permutations)
    if not 0 <= permutations < MAX_PROBLEMS:
        raise ValueError("%s: permutations must be in [0, %d)" % (what, MAX_PROBLEMS))
    chunk_rows = _chunk(what, chunk_rows)
    eval_only(what, model)
    xa = gather_codes(what, model, batches_a, space, chunk_rows)[0]
    xb = gather_codes(what, model, batches_b, space, chunk_rows)[0]
    if isinstance(gamma, str):
        gamma = median_bandwidth(xa, xb)                             # once, for both statistics
    out = [mmd2(xa, xb, kernel, gamma, degree, coef0, unbiased, scales).reshape(1)]
    if permutations:
        out.append(_permutation_stats(what, xa, xb, kernel, gamma, degree, coef0, scales, permutations, seed, None))
    flat = torch.cat(out).cpu().numpy().tolist()
    res = dict(mmd2=flat[0], n_a=xa.shape[0], n_b=xb.shape[0])
    if permutations:
        res.update(statistic=flat[1], p_value=p_value_of(flat[1:]))
    return res


def evaluate_prior_match(model, batches, samples=1, key=0, kernel="rbf", gamma="median", scales=None, unbiased=True, seed=0,
                         chunk_rows=256):
    """How far is the aggregate posterior of `model` from its N(0, I) prior, by samples?  The MMD^2 between z ~ q(z | x_i) -- `samples`
    draws per image, drawn as AggregatePosterior.sample draws them with `key` at row0 = the running index of the image -- and the
    prior: the WAE / InfoVAE regulariser as a diagnostic, the sample-based twin of evaluate_aggregate's marginal_kl.  Under "rbf" the
    prior side is analytic (rbf_prior_expectations: no prior draw, no sampling error on that side); under "imq" as many prior draws
    as there are codes stand in (torch.randn under a device generator seeded with `seed`).  "median": the bandwidth of the codes alone.
    -> mmd2, n, analytic.  One host read."""
    what = "evaluate_prior_match"
    latent_family(what, model)
    if kernel not in ("rbf", "imq"):
        raise ValueError("%s: kernel must be 'rbf' or 'imq' (a polynomial kernel sees a few moments only)" % what)
    _check_gamma(what, kernel, gamma, scales)
    samples = int(samples)
    if samples < 1 or samples > 65536:
        raise ValueError("%s: samples must be in [1, 65536]" % what)
    if key is None:
        raise ValueError("%s: the samples need a key" % what)
    chunk_rows = _chunk(what, chunk_rows)
    eval_only(what, model)
    mu, ls, _ = gather_codes(what, model, batches, "mu", chunk_rows)
    agg = AggregatePosterior(mu.shape[1])
    z = torch.cat([agg.sample(mu, ls, key=key, row0=0, s=s)[0] for s in range(samples)])
    n, D = z.shape
    if unbiased and n < 2:
        raise ValueError("%s: the unbiased statistic needs two codes" % what)
    kparam = kernel_params(kernel, gamma, D, z.device, 1.0, scales, (z,), what)
    if kernel == "rbf":
        szz = _scan(what, L.KSUM_RBF, kparam, 1, z, z, None, 0 if unbiased else -1, True)[1][0]
        exy, eyy = rbf_prior_expectations(z, kparam)
        val = szz / (n * (n - 1) if unbiased else n * n) - 2.0 * exy.sum() / n + eyy
    else:
        gen = torch.Generator(device=z.device).manual_seed(int(seed))
        prior = torch.randn(n, D, generator=gen, device=z.device, dtype=torch.float32)
        val = _mmd2_of(L.KSUM_IMQ, kparam, 1, z, prior, bool(unbiased))[0]
    return dict(mmd2=float(val.cpu().numpy()), n=n, analytic=kernel == "rbf")


def evaluate_kid(model, batches, source="generate", space="mu", subsets=100, subset_size=1000, degree=3, gamma=None, coef0=1.0, seed=0,
                 key=0, tau=1.0, mixture=None, chunk_rows=256):
    """The kernel inception distance of what `model` generates against the images of `batches` ((image, label) tuples on the device,
    regrouped to chunk_rows rows), with evaluate_generation's sources -- "generate": as many class-conditional samples as there are
    images, with the data's labels in order, drawn with `key` and `tau` at row0 = the running index; "reconstruct": the reconstructions
    of the same images; "mixture": the codes drawn from `mixture` (a fitted GaussianMixture) -- and spaces ("mu": the posterior means,
    "features": the pooled encoder features of a VariationalAutoEncoder).  -> kid()'s result and n.  One host read."""
    what = "evaluate_kid"
    _space(what, model, space)
    if source not in ("generate", "reconstruct", "mixture"):
        raise ValueError("%s: source must be 'generate', 'reconstruct' or 'mixture'" % what)
    if (source == "mixture") != (mixture is not None):
        raise ValueError("%s: source='mixture' needs a fitted mixture, and only that source takes one" % what)
    if key is None:
        raise ValueError("%s: the samples need a key" % what)
    chunk_rows = _chunk(what, chunk_rows)
    eval_only(what, model)

    def rows_of(image):
        return model.features(image).float().contiguous() if space == "features" else encode_posterior(model, image)[0]

    real, fake, count = [], [], 0
    for image, label in regroup(what, batches, chunk_rows):
        label = label.reshape(-1).long()
        if source == "mixture":
            from .mixture import generate_from_mixture
            made = generate_from_mixture(model, mixture, label, key, row0=count)
        elif source == "generate":
            made = model.generate(label, key, tau=tau, row0=count)
        else:
            made = model.reconstruct(image)
        real.append(rows_of(image))
        fake.append(rows_of(made))
        count += image.shape[0]
    if not real:
        raise ValueError("%s: the dataset is empty" % what)
    res = kid(torch.cat(real), torch.cat(fake), subsets, subset_size, degree, gamma, coef0, seed)
    res["n"] = count
    return res
