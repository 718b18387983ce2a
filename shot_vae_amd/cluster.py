"""Do the classes form clusters in latent space, and does the discrete posterior find them without the label?  Fused k-means and the
comparison of two partitions, on the HIP path (csrc/cluster.hip).

    km = KMeans(10, 128, seed=0).fit(mu)                               # k-means++ seeding, Lloyd iterations
    cluster = km.predict(mu)                                           # int64 [n] on the device
    table = contingency(label, cluster, 10, 10)                        # int64 [10, 10] on the device
    partition_metrics(table)                                           # accuracy (best matching), nmi, ari, purity, ...
    evaluate_clustering(model, loader, method="posterior")             # the model's own discrete code against the labels
    evaluate_clustering(model, loader, method="kmeans")                # plain k-means on the posterior means

Squared Euclid only.  The 2-Wasserstein distance of diagonal Gaussians is the squared Euclid distance of the concatenated rows
[mu, exp(ls)]: cluster torch.cat([mu, ls.exp()], 1) for it.  Rows must be finite: a NaN or infinite row is assigned to no cluster (-1)
and enters no centroid.  The [rows, centroids] matrix is never stored, there is no float atomic -- the same call sequence gives the same
bits --, nothing here synchronises with the host except where stated, and there is no CPU fallback."""
import numpy as np
import torch

from . import _lib as L
from .aggregate import partials
from ._latent import (LDS_PER_CU, _p, _st, eval_only, gather_codes, latent_family, matrix, num_classes, on_device, resident_partials,
                      split_batch, take_args)

MAX_CLUSTERS = 1024           # sv_kmeans_accum keeps [K][slice] doubles in LDS
MAX_CELLS = 1 << 20           # sv_contingency


def _slice(k):
    """the dimensions a block of sv_kmeans_accum owns: its [k][slice] double accumulators stay within 128 KiB of LDS"""
    return 64 if k <= 256 else 32 if k <= 512 else 16


def _partials(k, dim, n):
    """P of sv_kmeans_accum for n rows: aggregate.partials' rule over its grid of ceil(dim / slice) + 1 blocks per state -- every block
    weighed by the share of a compute unit its LDS takes (a quarter at the least: the four blocks per CU that rule aims at) --, lowered
    until the grid is resident at once (resident_partials).  A function of the shapes alone."""
    blocks = -(-dim // _slice(k)) + 1
    per_cu = max(1, min(4, LDS_PER_CU // (k * _slice(k) * 8)))
    return resident_partials(partials(blocks * 4 // per_cu, n), blocks, per_cu)


def _matrix(what, x, dim=None, k=None):
    """_latent.matrix for the clusterer; k: that many centroids are to be drawn from the rows"""
    def limit(n):
        if k is not None and not 1 <= k <= n:
            raise ValueError("%s: k = %d centroids from %d rows (k > N or k < 1)" % (what, k, n))
    return matrix(what, x, dim, "the clusterer", limit)


def _assign(x, c, want_dist=True):
    n, k = x.shape[0], c.shape[0]
    assign = torch.empty(n, dtype=torch.int64, device=x.device)
    dist = torch.empty(n, dtype=torch.float32, device=x.device) if want_dist else None
    L.call("sv_kmeans_assign", _p(x), n, _p(c), k, x.shape[1], _p(assign), _p(dist), _st())
    return assign, dist


def kmeans_plus_plus(x, k, u):
    """D^2 seeding (Arthur & Vassilvitskii 2007) as a deterministic function of the uniforms u (float64 [k], values in [0, 1)):
    the first centroid is row floor(u[0] n); centroid j is the first row whose running sum of min-distances, in float64, exceeds
    u[j] times the total -- a row at distance 0 from a chosen centroid is never drawn again.  The running minimum distance comes from
    sv_kmeans_assign against the newest centroid; the draw is torch.cumsum + searchsorted on the device: no host synchronisation.
    -> (centroids fp32 [k, d], the chosen row indices int64 [k])"""
    k = int(k)
    x = _matrix("kmeans_plus_plus", x, k=k)
    n = x.shape[0]
    if torch.is_tensor(u) and not u.is_cuda:
        u = u.to(x.device)
    if not torch.is_tensor(u) or u.dtype != torch.float64 or tuple(u.shape) != (k,):
        raise ValueError("kmeans_plus_plus: u must be a float64 vector [%d]" % k)
    idx = torch.empty(k, dtype=torch.int64, device=x.device)
    idx[0] = torch.clamp((u[0] * n).floor().long(), 0, n - 1)
    mind = torch.full((n,), float("inf"), dtype=torch.float32, device=x.device)
    for j in range(1, k):
        newest = x.index_select(0, idx[j - 1:j])
        mind = torch.minimum(mind, _assign(x, newest)[1])
        cum = torch.cumsum(mind.double(), 0)
        idx[j] = torch.clamp(torch.searchsorted(cum, (u[j] * cum[-1]).reshape(1), right=True)[0], 0, n - 1)
    return x.index_select(0, idx), idx


class KMeans:
    """Lloyd's k-means on device rows [n, dim], one iteration = sv_kmeans_assign, sv_kmeans_accum, sv_kmeans_finish.

    init: "k-means++" (kmeans_plus_plus with uniforms from a torch.Generator seeded with `seed`), "random" (k distinct rows, the same
    generator) or a tensor [k, dim] of starting centroids.  An empty cluster keeps its centroid.  step() and predict() issue no host
    synchronisation and can be captured under torch.cuda.graph and replayed on new rows of the same shape."""

    def __init__(self, k, dim, init="k-means++", seed=0):
        self.k, self.dim, self.seed = int(k), int(dim), int(seed)
        if not 1 <= self.k <= MAX_CLUSTERS:
            raise ValueError("KMeans: k must be in [1, %d] (sv_kmeans_accum's accumulators live in LDS); got %d" % (MAX_CLUSTERS, self.k))
        if self.dim < 1:
            raise ValueError("KMeans: dim must be >= 1")
        if torch.is_tensor(init):
            if tuple(init.shape) != (self.k, self.dim):
                raise ValueError("KMeans: init must be a tensor [%d, %d], not %s" % (self.k, self.dim, list(init.shape)))
            if not init.is_cuda:
                raise L.ShotVaeHipError("KMeans: init is not on an MI355X (no CPU fallback)")
        elif init not in ("k-means++", "random"):
            raise ValueError("KMeans: init must be 'k-means++', 'random' or a tensor [k, dim]")
        self.init = init
        self.centroids = self.counts = self.inertia = self.stats = None
        self.n_iter = 0

    def _start(self, x, gen):
        if torch.is_tensor(self.init):
            return self.init.detach().float().contiguous().clone()
        if self.init == "random":
            return x.index_select(0, torch.randperm(x.shape[0], generator=gen)[:self.k].to(x.device))
        return kmeans_plus_plus(x, self.k, torch.rand(self.k, dtype=torch.float64, generator=gen).to(x.device))[0]

    def _lloyd(self, x, c_old, c_new):
        """one assignment of x to c_old and the centroids of that assignment into c_new (may be c_old) -> (count, stats)"""
        n, dev = x.shape[0], x.device
        P = _partials(self.k, self.dim, n)
        assign, dist = _assign(x, c_old)
        sums = torch.empty(P, self.k, self.dim, dtype=torch.float64, device=dev)
        counts = torch.empty(P, self.k, dtype=torch.int64, device=dev)
        inertia = torch.empty(P, dtype=torch.float64, device=dev)
        count = torch.empty(self.k, dtype=torch.int64, device=dev)
        stats = torch.empty(2, dtype=torch.float32, device=dev)
        L.call("sv_kmeans_accum", _p(x), _p(assign), _p(dist), n, self.dim, self.k, _p(sums), _p(counts), _p(inertia), P, 1, _st())
        L.call("sv_kmeans_finish", _p(sums), _p(counts), _p(inertia), P, self.k, self.dim, _p(c_old), _p(c_new), _p(count), _p(stats), _st())
        return count, stats

    def step(self, x):
        """one Lloyd iteration from the current centroids, in place -> stats fp32 [2] on the device: the squared shift of the centroids
        and the inertia of x about the centroids the step STARTED from.  self.counts = the cluster sizes of that assignment."""
        x = _matrix("KMeans.step", x, self.dim)
        if self.centroids is None:
            raise ValueError("KMeans.step: no centroids yet: call fit(), or construct with init = a tensor and call reset()")
        self.counts, self.stats = self._lloyd(x, self.centroids, self.centroids)
        self.n_iter += 1
        return self.stats

    def reset(self, x=None, generator=None):
        """(re)places the centroids at their initial position: the init tensor, or a seeding of the rows x"""
        if not torch.is_tensor(self.init):
            x = _matrix("KMeans.reset", x, self.dim, k=self.k)
        gen = generator if generator is not None else torch.Generator().manual_seed(self.seed)
        self.centroids = self._start(x, gen)
        self.n_iter = 0
        return self

    def fit(self, x, max_iter=100, tol=1e-4, check_every=1, n_init=1):
        """Lloyd iterations until the squared shift of the centroids, stats[0], is <= tol x the mean per-dimension (population)
        variance of x -- scikit-learn's rule -- or max_iter is reached.  stats is read on the host once per `check_every` iterations
        (and the variance once); tol=None never reads: exactly max_iter iterations.  n_init > 1 repeats the run with further draws
        of the same generator and keeps the run of least inertia (chosen on the device).  Afterwards centroids [k, dim], counts int64
        [k] and inertia (fp32 scalar tensor) describe x about the FINAL centroids (one more assignment), n_iter the iterations of the
        last run."""
        max_iter, check_every, n_init = int(max_iter), int(check_every), int(n_init)
        if max_iter < 1 or check_every < 1 or n_init < 1:
            raise ValueError("KMeans.fit: max_iter, check_every and n_init must be >= 1")
        x = _matrix("KMeans.fit", x, self.dim, k=None if torch.is_tensor(self.init) else self.k)
        gen = torch.Generator().manual_seed(self.seed)
        bound = None
        best = None
        for _ in range(n_init):
            self.reset(x, gen)
            for it in range(1, max_iter + 1):
                stats = self.step(x)
                if tol is not None and (it % check_every == 0 or it == max_iter):
                    if bound is None:
                        bound = float(tol) * float(x.double().var(dim=0, unbiased=False).mean())
                    if float(stats.cpu()[0]) <= bound:
                        break
            scratch = torch.empty_like(self.centroids)
            count, stats = self._lloyd(x, self.centroids, scratch)
            run = (self.centroids, count, stats[1].clone())
            if best is None:
                best = run
            else:
                better = run[2] < best[2]
                best = tuple(torch.where(better, a, b) for a, b in zip(run, best))
        self.centroids, self.counts, self.inertia = best
        return self

    def predict(self, x, return_distance=False):
        """-> the nearest centroid of every row, int64 [n] (the smaller index on a tie; -1 for a row that is not finite);
        return_distance: -> (cluster, squared distance fp32 [n])"""
        x = _matrix("KMeans.predict", x, self.dim)
        if self.centroids is None:
            raise ValueError("KMeans.predict: no centroids yet: call fit() first")
        assign, dist = _assign(x, self.centroids, want_dist=return_distance)
        return (assign, dist) if return_distance else assign


def contingency(a, b, ka, kb):
    """-> int64 [ka, kb] on the device: [i, j] = the number of rows with a == i and b == j (a, b: int64 label vectors of one length on
    the device; a row with either label out of range is in no cell).  sv_contingency: integer atomics only, no host synchronisation."""
    on_device("contingency", a, b)
    if not torch.is_tensor(a) or not torch.is_tensor(b) or a.dtype != torch.int64 or b.dtype != torch.int64 or a.dim() != 1 \
            or a.shape != b.shape or a.numel() < 1:
        raise ValueError("contingency: a and b must be non-empty int64 vectors of one length")
    ka, kb = int(ka), int(kb)
    if ka < 1 or kb < 1 or ka * kb > MAX_CELLS:
        raise ValueError("contingency: ka, kb must be >= 1 and ka * kb <= 2^20")
    a, b = a.contiguous(), b.contiguous()
    table = torch.zeros(ka, kb, dtype=torch.int64, device=a.device)
    counts = torch.zeros(2, dtype=torch.int64, device=a.device)
    L.call("sv_contingency", _p(a), _p(b), a.numel(), ka, kb, _p(table), _p(counts), _st())
    return table


def linear_assignment(cost):
    """The minimum-cost one-to-one assignment of a real cost matrix [n, m] on the host (numpy; the shortest-augmenting-path form of the
    Hungarian method with potentials, Jonker & Volgenant 1987, O(min(n, m)^2 max(n, m))): -> (rows, cols) int64 [min(n, m)], rows
    ascending, as scipy.optimize.linear_sum_assignment returns them."""
    cost = np.asarray(cost, dtype=np.float64)
    if cost.ndim != 2 or not np.isfinite(cost).all():
        raise ValueError("linear_assignment: cost must be a finite matrix")
    if cost.shape[0] == 0 or cost.shape[1] == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    if cost.shape[0] > cost.shape[1]:
        cols, rows = linear_assignment(cost.T)
        order = np.argsort(rows)
        return rows[order], cols[order]
    n, m = cost.shape
    u, v = np.zeros(n + 1), np.zeros(m + 1)
    match = np.zeros(m + 1, dtype=np.int64)            # match[j] = the row (1-based) assigned to column j; column 0 is the virtual root
    way = np.zeros(m + 1, dtype=np.int64)
    for i in range(1, n + 1):
        match[0] = i
        j0 = 0
        minv = np.full(m + 1, np.inf)
        used = np.zeros(m + 1, dtype=bool)
        while True:
            used[j0] = True
            i0 = match[j0]
            cur = cost[i0 - 1] - u[i0] - v[1:]
            free = ~used[1:]
            upd = free & (cur < minv[1:])
            minv[1:][upd] = cur[upd]
            way[1:][upd] = j0
            cand = np.where(free, minv[1:], np.inf)
            j1 = int(np.argmin(cand)) + 1
            delta = cand[j1 - 1]
            u[match[used]] += delta
            v[used] -= delta
            minv[1:][free] -= delta
            j0 = j1
            if match[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            match[j0] = match[j1]
            j0 = j1
    cols = np.nonzero(match[1:])[0]
    rows = match[1:][cols] - 1
    order = np.argsort(rows)
    return rows[order].astype(np.int64), cols[order].astype(np.int64)


def _entropy(p):
    p = p[p > 0]
    return float(-(p * np.log(p)).sum())


def partition_metrics(table):
    """How well do two partitions of the same rows agree?  table [Ka, Kb]: rows = the reference partition (classes), columns = the
    clusters; a device tensor (ONE host read) or a numpy array; rectangular tables are fine.  Float64 on the host:

        accuracy      the share of rows on the best one-to-one matching of clusters to classes (linear_assignment)
        mapping       int64 [Kb]: the class matched to each cluster, -1 for an unmatched cluster
        purity        the share of rows in the largest class of their cluster
        nmi           I(a; b) / ((H(a) + H(b)) / 2): the arithmetic normalisation; 1 when both partitions are a single block
        ari           the adjusted Rand index (Hubert & Arabie 1985), from the pair counts; 1 when the partitions are identical
        homogeneity   1 - H(a | b) / H(a)      (1 when H(a) = 0)
        completeness  1 - H(b | a) / H(b)      (1 when H(b) = 0)
        v_measure     their harmonic mean (Rosenberg & Hirschberg 2007)
        n             the number of rows in the table"""
    if torch.is_tensor(table):
        table = table.detach().cpu().numpy()
    t = np.asarray(table)
    if t.ndim != 2 or t.shape[0] < 1 or t.shape[1] < 1 or (t < 0).any():
        raise ValueError("partition_metrics: a non-negative table [Ka, Kb]")
    t = t.astype(np.int64)
    n = int(t.sum())
    if n < 1:
        raise ValueError("partition_metrics: the table is empty")
    rows, cols = linear_assignment(-t.astype(np.float64))
    mapping = np.full(t.shape[1], -1, dtype=np.int64)
    mapping[cols] = rows
    a, b = t.sum(axis=1), t.sum(axis=0)
    ha, hb = _entropy(a / n), _entropy(b / n)
    nz = t > 0
    mi = float((t[nz] / n * (np.log(t[nz].astype(np.float64)) + np.log(n) - np.log(np.outer(a, b)[nz].astype(np.float64)))).sum())
    mi = max(mi, 0.0)
    # decided on the integers, so that no rounding of a logarithm stands between a perfect partition and 1: H(a | b) = 0 exactly when
    # every cluster lies inside one class, H(b | a) = 0 when every class lies inside one cluster
    pure_cols, pure_rows = bool(((t > 0).sum(axis=0) <= 1).all()), bool(((t > 0).sum(axis=1) <= 1).all())
    hom = 1.0 if pure_cols else mi / ha
    com = 1.0 if pure_rows else mi / hb
    nmi = 1.0 if pure_cols and pure_rows else mi / (0.5 * (ha + hb))
    # pair counts as Python integers: exact for any n
    pairs = lambda v: sum(int(c) * (int(c) - 1) // 2 for c in np.ravel(v))          # noqa: E731
    tp = pairs(t)
    fp, fn = pairs(b) - tp, pairs(a) - tp
    tn = n * (n - 1) // 2 - tp - fp - fn
    ari = 1.0 if fp == 0 and fn == 0 else 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    return dict(accuracy=float(t[rows, cols].sum()) / n, mapping=mapping, purity=float(t.max(axis=0).sum()) / n, nmi=nmi, ari=ari,
                homogeneity=hom, completeness=com, v_measure=0.0 if hom + com == 0.0 else 2.0 * hom * com / (hom + com), n=n)


def evaluate_clustering(model, data, method="posterior", k=None, space="mu", **kmeans_args):
    """Do the classes of `data` ((image, label) batches on the device) form clusters in the latent space of `model` (a
    VariationalAutoEncoder or a SmoothVAE, in eval mode: NotImplementedError otherwise, as for score)?  The label is used for scoring only.

        method  "posterior"   the cluster of an image is the first maximum of its discrete posterior q(y | x) (disc_log_alpha / alphas):
                              what the model's categorical code finds on its own; k = the number of classes of the code
                "kmeans"      KMeans(k, **kmeans_args: init, seed, and fit's max_iter, tol, check_every, n_init) on the posterior means
                              (encode_posterior) of the whole set: what plain k-means finds in the continuous code; k defaults to the
                              number of classes of the discrete code
        space   "mu"          the posterior means (the only space: for W2 cluster [mu, exp(ls)] with KMeans yourself)

    Labels outside [0, number of classes of the code) are in no cell.  The rows are gathered over the batches before anything is
    clustered: the result does not depend on the batching.  -> partition_metrics of the contingency table (classes x clusters), plus
    `counts` (int64 numpy [k]: the size of every cluster) and `clusters` (int64 [n] on the device: the cluster of every image, in order).
    One host read at the end (k-means with a tolerance adds its convergence checks)."""
    latent_family("evaluate_clustering", model)
    if method not in ("posterior", "kmeans"):
        raise ValueError("evaluate_clustering: method must be 'posterior' or 'kmeans'")
    if space != "mu":
        raise ValueError("evaluate_clustering: space must be 'mu'")
    if method == "posterior" and (k is not None or kmeans_args):
        raise ValueError("evaluate_clustering: method='posterior' takes no k and no k-means arguments (k is the size of the discrete code)")
    eval_only("evaluate_clustering", model)
    fit_args = take_args(kmeans_args, ("max_iter", "tol", "check_every", "n_init"))
    classes = num_classes(model)

    if method == "posterior":
        rows, labels = [], []
        for batch in data:
            image, label = split_batch("evaluate_clustering", batch, True)
            with torch.no_grad():
                rows.append(model.encode(image)[2].argmax(dim=1))      # log alpha (SHOT-VAE) or alpha (smooth): the same first maximum
            labels.append(label)
        if not rows:
            raise ValueError("evaluate_clustering: the dataset is empty")
        k, cluster, label = classes, torch.cat(rows), torch.cat(labels)
    else:
        mu, _, label = gather_codes("evaluate_clustering", model, data)
        k = classes if k is None else int(k)
        cluster = KMeans(k, mu.shape[1], **kmeans_args).fit(mu, **fit_args).predict(mu)
    table = contingency(label, cluster, classes, k)
    sizes = contingency(torch.zeros_like(cluster), cluster, 1, k)          # (every image, whatever its label)
    host = torch.cat([table.reshape(-1), sizes.reshape(-1)]).cpu().numpy()
    res = partition_metrics(host[:classes * k].reshape(classes, k))
    res.update(counts=host[classes * k:], clusters=cluster)
    return res
