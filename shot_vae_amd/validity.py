"""How many clusters are there, and how well separated are the classes in latent space?  Internal cluster validity on the HIP path
(csrc/validity.hip): the silhouette (Rousseeuw 1987), the Calinski-Harabasz index and the Davies-Bouldin index -- no label
needed, unlike cluster.partition_metrics.

    s = silhouette_samples(mu, cluster, 10)                            # float64 [n] on the device, the caller's row order
    silhouette_score(mu, cluster, 10)                                  # score, per_cluster, counts, skipped
    validity_indices(mu, cluster, 10)                                  # silhouette, calinski_harabasz, davies_bouldin
    evaluate_validity(model, loader, method="labels")                  # how separated are the true classes in this space?
    evaluate_validity(model, loader, method="kmeans", k=[2, 5, 10, 20])    # the "how many clusters" sweep: best_k by silhouette

Metrics "euclid" and "sqeuclid".  A label outside [0, k) or a row that is not finite belongs to no cluster: it enters no other row's
sums and its own silhouette is NaN (counted in `skipped`).  The [n, n] distance matrix is never stored, there is no atomic -- the same
call gives the same bits --, nothing here synchronises with the host except where stated, and there is no CPU fallback."""
import numpy as np
import torch

from . import _lib as L
from ._latent import _p, _st, eval_only, gather_codes, latent_family, matrix, num_classes, on_device, regroup, take_args
from ._latent import labels as _labels
from .aggregate import partials
from .cluster import MAX_CLUSTERS, KMeans, _partials as _kmeans_partials

METRICS = {"euclid": L.SIL_EUCLID, "sqeuclid": L.SIL_SQEUCLID}
MAX_PARTIALS = 64


def _metric(what, metric):
    if metric not in METRICS:
        raise ValueError("%s: unknown metric %r (one of 'euclid', 'sqeuclid')" % (what, metric))
    return METRICS[metric]


def _k(what, k):
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= MAX_CLUSTERS:
        raise ValueError("%s: k must be an integer in [1, %d]" % (what, MAX_CLUSTERS))
    return int(k)


def default_partials(q, n, k):
    """P of sv_sil_scan for q query rows against n gallery rows in k clusters: aggregate.partials' rule, never more states than
    clusters.  A function of the shapes alone (s does not depend on it)."""
    return min(k, partials(-(-q // 64), n))


# ---- the two raw launches ----
def silhouette_grouped(q, q_label, g, seg, k, metric="euclid", P=None):
    """sv_sil_scan + sv_sil_finish on rows that are already grouped: q fp32 [Q, D] with q_label int64 [Q], the gallery g fp32 [N, D]
    whose rows seg[c] .. seg[c + 1] - 1 are cluster c (seg int64 [k + 1] on the device; every bound is clipped to [0, N]).  A query
    with a label in [0, k) is taken to be one of the gallery's rows.  -> (s float64 [Q], cluster_sum float64 [k], cluster_cnt int64 [k],
    skipped int64 [1]) on the device: the silhouette of every query (NaN: no value), per cluster the sum and the number of the values,
    and the number of NaNs.  No host synchronisation: capturable under torch.cuda.graph and replayable on new rows and a new seg of
    the same shapes.  P (the partial states; default_partials) changes no bit of the result."""
    what = "silhouette_grouped"
    code, k = _metric(what, metric), _k(what, k)
    for name, t in (("q", q), ("g", g)):
        if not torch.is_tensor(t) or t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1 or t.dtype != torch.float32:
            raise ValueError("%s: %s must be a non-empty fp32 matrix [rows, d]" % (what, name))
    if q.shape[1] != g.shape[1]:
        raise ValueError("%s: q has %d columns, g %d" % (what, q.shape[1], g.shape[1]))
    if not torch.is_tensor(q_label) or q_label.dtype != torch.int64 or tuple(q_label.shape) != (q.shape[0],):
        raise ValueError("%s: q_label must be an int64 vector [%d]" % (what, q.shape[0]))
    if not torch.is_tensor(seg) or seg.dtype != torch.int64 or tuple(seg.shape) != (k + 1,):
        raise ValueError("%s: seg must be an int64 vector [k + 1 = %d]" % (what, k + 1))
    Q, D, N = q.shape[0], q.shape[1], g.shape[0]
    P = default_partials(Q, N, k) if P is None else int(P)
    if not 1 <= P <= MAX_PARTIALS:
        raise ValueError("%s: P must be in [1, %d]" % (what, MAX_PARTIALS))
    on_device(what, q, q_label, g, seg)
    q, q_label, g, seg = q.contiguous(), q_label.contiguous(), g.contiguous(), seg.contiguous()
    dev = q.device
    part = torch.empty(2, P, Q, dtype=torch.float64, device=dev)
    s = torch.empty(Q, dtype=torch.float64, device=dev)
    csum = torch.empty(k, dtype=torch.float64, device=dev)
    ccnt = torch.empty(k, dtype=torch.int64, device=dev)
    skipped = torch.empty(1, dtype=torch.int64, device=dev)
    L.call("sv_sil_scan", code, _p(q), _p(q_label), Q, _p(g), _p(seg), N, k, D, P, _p(part[0]), _p(part[1]), _st())
    L.call("sv_sil_finish", _p(part[0]), _p(part[1]), P, Q, _p(q_label), _p(seg), k, N, _p(s), None, None, _p(csum), _p(ccnt), _p(skipped),
           _st())
    return s, csum, ccnt, skipped


# ---- grouping ----
def _group(what, x, y, k):
    """-> (key int64 [n]: the row's cluster, k for a row that belongs to none; order int64 [n]: the stable sort of key; seg int64
    [k + 1]: cluster c is rows seg[c] .. seg[c + 1] - 1 of x[order]; what belongs to no cluster sorts behind seg[k]).  Device only."""
    key = torch.where((y >= 0) & (y < k) & torch.isfinite(x).all(dim=1), y, torch.full_like(y, k))
    skey, order = torch.sort(key, stable=True)
    seg = torch.searchsorted(skey, torch.arange(k + 1, dtype=torch.int64, device=x.device))
    return key, order, seg


def _check(what, x, labels, k, metric, queries):
    _metric(what, metric)
    k = _k(what, k)
    if not torch.is_tensor(x) or x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError("%s: x must be a non-empty matrix [n, d]" % what)
    n = x.shape[0]
    if not torch.is_tensor(labels) or labels.dim() != 1 or labels.shape[0] != n or labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise ValueError("%s: labels must be an integer vector [%d]" % (what, n))
    if queries is not None and (isinstance(queries, bool) or int(queries) != queries or not 1 <= int(queries) <= n):
        raise ValueError("%s: queries must be None or an integer in [1, n = %d]" % (what, n))
    return matrix(what, x), _labels(what, labels, n), k, None if queries is None else int(queries)


def query_indices(n, m, seed):
    """the row subset of queries=m: the first m entries of torch.randperm(n) under a CPU generator seeded with `seed` -> int64 [m], CPU"""
    return torch.randperm(n, generator=torch.Generator().manual_seed(int(seed)))[:m]


def _samples(what, x, y, k, metric, queries, seed):
    """-> (s in the caller's order (or the subset's), the subset's indices or None, grouped's cluster_sum, cluster_cnt, skipped, seg)"""
    key, order, seg = _group(what, x, y, k)
    g = x.index_select(0, order)
    if queries is None:
        s_sorted, csum, ccnt, skipped = silhouette_grouped(g, key.index_select(0, order), g, seg, k, metric)
        s = torch.empty_like(s_sorted)
        s[order] = s_sorted
        return s, None, csum, ccnt, skipped, seg
    idx = query_indices(x.shape[0], queries, seed).to(x.device)
    s, csum, ccnt, skipped = silhouette_grouped(x.index_select(0, idx), key.index_select(0, idx), g, seg, k, metric)
    return s, idx, csum, ccnt, skipped, seg


def silhouette_samples(x, labels, k, metric="euclid", queries=None, seed=0):
    """The silhouette s_i = (b_i - a_i) / max(a_i, b_i) of every row of x [n, d] under the partition `labels` (int64 [n], clusters 0 ..
    k - 1): a_i the mean distance to the other rows of its cluster, b_i the smallest mean distance to the rows of another cluster; 0
    for a singleton, scikit-learn's conventions.  The rows are grouped by a stable device sort; a label outside [0, k) or a row that
    is not finite belongs to no cluster (NaN, and in no other row's sums); with fewer than two non-empty clusters every value is NaN.
    -> float64 [n] on the device in the caller's row order, no host read.

    queries=m scores a seeded subset of m rows (query_indices) against the FULL gallery: an estimate of the mean at m / n of the cost,
    every value exact.  This is deliberately not scikit-learn's sample_size, which also thins the gallery and so changes every a_i
    and b_i.  -> (float64 [m], the subset's row indices int64 [m]), both on the device."""
    what = "silhouette_samples"
    x, y, k, queries = _check(what, x, labels, k, metric, queries)
    s, idx = _samples(what, x, y, k, metric, queries, seed)[:2]
    return s if queries is None else (s, idx)


def _score_of(host, k):
    """(score, per_cluster, counts, skipped) from the host vector [cluster_sum k | cluster_cnt k | sizes k | skipped 1] (float64)"""
    csum, ccnt, sizes, skipped = host[:k], host[k:2 * k].astype(np.int64), host[2 * k:3 * k].astype(np.int64), int(host[3 * k])
    if int((sizes > 0).sum()) < 2:
        raise ValueError("the silhouette needs at least 2 non-empty clusters, there %s %d" % (
            "is" if int((sizes > 0).sum()) == 1 else "are", int((sizes > 0).sum())))
    with np.errstate(invalid="ignore", divide="ignore"):
        per = np.where(ccnt > 0, csum / ccnt, np.nan)
        score = float(csum.sum() / ccnt.sum()) if ccnt.sum() > 0 else float("nan")
    return score, per, sizes, skipped


def _pack(csum, ccnt, skipped, seg):
    return [csum, ccnt.double(), (seg[1:] - seg[:-1]).double(), skipped.double()]


def silhouette_score(x, labels, k, metric="euclid", queries=None, seed=0):
    """The mean silhouette over the rows that have one (silhouette_samples; queries=m: over a seeded subset against the full gallery).
    -> score, per_cluster (float64 numpy [k]: the mean over each cluster's scored rows, NaN for none), counts (int64 numpy [k]: the
    cluster sizes), skipped (the scored rows without a value).  Fewer than 2 non-empty clusters: ValueError, as in scikit-learn.  One
    host read."""
    what = "silhouette_score"
    x, y, k, queries = _check(what, x, labels, k, metric, queries)
    _, _, csum, ccnt, skipped, seg = _samples(what, x, y, k, metric, queries, seed)
    score, per, sizes, skip = _score_of(torch.cat(_pack(csum, ccnt, skipped, seg)).cpu().numpy(), k)
    return dict(score=score, per_cluster=per, counts=sizes, skipped=skip)


# ---- Calinski-Harabasz and Davies-Bouldin ----
def _spread(what, x, y, k):
    """device tensors: centroids fp32 [k, d] (zeros for an empty cluster), counts int64 [k], stat float64 [k, 2] = (sum of squared
    distances to the own centroid, sum of distances)"""
    n, D, dev = x.shape[0], x.shape[1], x.device
    assign = torch.where((y >= 0) & (y < k) & torch.isfinite(x).all(dim=1), y, torch.full_like(y, -1))
    P = _kmeans_partials(k, D, n)
    sums = torch.empty(P, k, D, dtype=torch.float64, device=dev)
    counts = torch.empty(P, k, dtype=torch.int64, device=dev)
    zero = torch.zeros(k, D, dtype=torch.float32, device=dev)
    cent = torch.empty(k, D, dtype=torch.float32, device=dev)
    count = torch.empty(k, dtype=torch.int64, device=dev)
    shift = torch.empty(2, dtype=torch.float32, device=dev)
    L.call("sv_kmeans_accum", _p(x), _p(assign), None, n, D, k, _p(sums), _p(counts), None, P, 1, _st())
    L.call("sv_kmeans_finish", _p(sums), _p(counts), None, P, k, D, _p(zero), _p(cent), _p(count), _p(shift), _st())
    stat = torch.empty(k, 2, dtype=torch.float64, device=dev)
    cnt = torch.empty(k, dtype=torch.int64, device=dev)
    L.call("sv_cluster_spread", _p(x), _p(assign), n, D, _p(cent), k, None, _p(stat), _p(cnt), _st())
    return cent, cnt, stat


def cluster_spread(x, labels, k):
    """The centroids of the partition `labels` of the rows x [n, d] and the spread about them, on the device without a host read:
    -> (centroids fp32 [k, d] -- sv_kmeans_accum + sv_kmeans_finish: double sums in a fixed order, zeros for an empty cluster --,
    counts int64 [k], within float64 [k]: the sum of squared distances to the own centroid, mean_dist float64 [k]: the mean distance
    to it, 0 for an empty cluster).  A label outside [0, k) or a row that is not finite belongs to no cluster."""
    what = "cluster_spread"
    x, y, k, _ = _check(what, x, labels, k, "euclid", None)
    cent, cnt, stat = _spread(what, x, y, k)
    return cent, cnt, stat[:, 0].contiguous(), torch.where(cnt > 0, stat[:, 1] / cnt.clamp(min=1).double(), torch.zeros_like(stat[:, 1]))


def _host_stats(centroids, counts, third):
    c = np.asarray(centroids, dtype=np.float64)
    n = np.asarray(counts).astype(np.int64).reshape(-1)
    t = np.asarray(third, dtype=np.float64).reshape(-1)
    if c.ndim != 2 or c.shape[0] != n.shape[0] or t.shape[0] != n.shape[0] or (n < 0).any():
        raise ValueError("centroids [k, d], counts [k] >= 0 and one value per cluster [k]")
    keep = n > 0
    return c[keep], n[keep], t[keep]


def calinski_harabasz(centroids, counts, within):
    """The Calinski-Harabasz index (variance ratio criterion) in float64 numpy from cluster_spread's results on the host: B (n - k) /
    (W (k - 1)), B = sum_c n_c |centroid_c - mean|^2 with the mean of all rows, W = sum_c within_c, over the k NON-EMPTY clusters;
    1.0 when W == 0 (scikit-learn's conventions).  Fewer than 2 non-empty clusters, or as many as rows: ValueError."""
    c, n, w = _host_stats(centroids, counts, within)
    rows, k = int(n.sum()), len(n)
    if not 2 <= k <= rows - 1:
        raise ValueError("calinski_harabasz: %d non-empty clusters for %d rows (2 .. rows - 1 are valid)" % (k, rows))
    mean = (n[:, None] * c).sum(axis=0) / rows
    extra = float((n * ((c - mean[None, :]) ** 2).sum(axis=1)).sum())
    intra = float(w.sum())
    return 1.0 if intra == 0.0 else extra * (rows - k) / (intra * (k - 1.0))


def davies_bouldin(centroids, counts, mean_dist):
    """The Davies-Bouldin index in float64 numpy from cluster_spread's results on the host: the mean over the NON-EMPTY clusters i of
    max_{j != i} (mean_dist_i + mean_dist_j) / |centroid_i - centroid_j| (direct differences); a ratio with zero centroid distance
    counts as 0, and the index is 0 when every spread or every centroid distance is (scikit-learn's conventions).  Fewer than 2
    non-empty clusters, or as many as rows: ValueError."""
    c, n, s = _host_stats(centroids, counts, mean_dist)
    rows, k = int(n.sum()), len(n)
    if not 2 <= k <= rows - 1:
        raise ValueError("davies_bouldin: %d non-empty clusters for %d rows (2 .. rows - 1 are valid)" % (k, rows))
    d = c[:, None, :] - c[None, :, :]
    m = np.sqrt((d * d).sum(axis=2))
    if np.allclose(s, 0.0) or np.allclose(m, 0.0):
        return 0.0
    m[m == 0.0] = np.inf
    ratio = (s[:, None] + s[None, :]) / m
    np.fill_diagonal(ratio, 0.0)
    return float(ratio.max(axis=1).mean())


def _indices(what, x, y, k, metric, queries, seed):
    """validity_indices on checked inputs -> the dict (one host read)"""
    _, _, csum, ccnt, skipped, seg = _samples(what, x, y, k, metric, queries, seed)
    cent, cnt, stat = _spread(what, x, y, k)
    D = x.shape[1]
    host = torch.cat(_pack(csum, ccnt, skipped, seg) + [stat.reshape(-1), cent.double().reshape(-1)]).cpu().numpy()
    score, per, sizes, skip = _score_of(host, k)
    stat_h = host[3 * k + 1:5 * k + 1].reshape(k, 2)
    cent_h = host[5 * k + 1:].reshape(k, D)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_dist = np.where(sizes > 0, stat_h[:, 1] / np.maximum(sizes, 1), 0.0)
    return dict(silhouette=score, calinski_harabasz=calinski_harabasz(cent_h, sizes, stat_h[:, 0]),
                davies_bouldin=davies_bouldin(cent_h, sizes, mean_dist), per_cluster=per, counts=sizes, skipped=skip,
                clusters=int((sizes > 0).sum()), n=int(sizes.sum()))


def validity_indices(x, labels, k, metric="euclid", queries=None, seed=0):
    """All three internal indices of the partition `labels` of the rows x [n, d]: -> silhouette (higher is better; `metric`, `queries`
    as in silhouette_score), calinski_harabasz (higher), davies_bouldin (lower; both on Euclid distances to the centroids), per_cluster,
    counts, skipped (silhouette_score's), clusters (the non-empty ones), n (the rows that belong to a cluster).  Needs 2 .. n - 1
    non-empty clusters (ValueError).  One host read."""
    what = "validity_indices"
    x, y, k, queries = _check(what, x, labels, k, metric, queries)
    return _indices(what, x, y, k, metric, queries, seed)


# ---- the evaluator ----
def evaluate_validity(model, data, method="labels", k=None, space="mu", queries=None, chunk_rows=None, metric="euclid", seed=0,
                      **kmeans_args):
    """Internal validity of a partition of the codes of `data` ((image, label) batches on the device) in the latent space of `model` (a
    VariationalAutoEncoder or a SmoothVAE, in eval mode: NotImplementedError otherwise).

        method  "labels"      the true classes as the partition: how separated are the classes in this space?  (k = the number of classes
                              of the discrete code; labels outside it belong to no cluster)
                "posterior"   the first maximum of the discrete posterior q(y | x): how compact is what the model's own code finds?
                "kmeans"      KMeans(k, seed=seed, **kmeans_args: init, and fit's max_iter, tol, check_every, n_init) on the same rows; k defaults to the number of classes and may be a LIST: the result is then
                              {results: one dict per k, ks, best_k: the k of the largest silhouette} -- the "how many clusters" sweep
        space   "mu"          the posterior means
                "w2"          the concatenated rows [mu, exp(ls)], whose Euclid distance is the 2-Wasserstein distance of the posteriors
                "features"    the pooled encoder features (a VariationalAutoEncoder only)

    The rows are gathered before anything is scored, regrouped to chunk_rows rows before the model sees them when chunk_rows is given:
    the result then does not depend on the batching.  seed: of the queries' subset and of k-means.  -> validity_indices' dict plus method, space and k.  One host read per scored
    partition (k-means with a tolerance adds its convergence checks)."""
    what = "evaluate_validity"
    family = latent_family(what, model)
    if method not in ("labels", "posterior", "kmeans"):
        raise ValueError("%s: method must be 'labels', 'posterior' or 'kmeans'" % what)
    if space not in ("mu", "w2", "features"):
        raise ValueError("%s: space must be 'mu', 'w2' or 'features'" % what)
    if space == "features" and family != "shot":
        raise ValueError("%s: space='features' needs a VariationalAutoEncoder (a SmoothVAE has no pooled features)" % what)
    _metric(what, metric)
    if method != "kmeans" and (k is not None or kmeans_args):
        raise ValueError("%s: method=%r takes no k and no k-means arguments (k is the size of the discrete code)" % (what, method))
    classes = num_classes(model)
    ks = None
    if method == "kmeans":
        ks = [_k(what, v) for v in k] if isinstance(k, (list, tuple)) else [classes if k is None else _k(what, k)]
        if not ks or len(set(ks)) != len(ks):
            raise ValueError("%s: k must name at least one number of clusters, none of them twice" % what)
    if chunk_rows is not None and int(chunk_rows) < 1:
        raise ValueError("%s: chunk_rows must be >= 1 or None" % what)
    chunk_rows = None if chunk_rows is None else int(chunk_rows)
    eval_only(what, model)
    fit_args = take_args(kmeans_args, ("max_iter", "tol", "check_every", "n_init"))

    data = list(data)
    x, ls, label = gather_codes(what, model, data, "features" if space == "features" else "mu", chunk_rows)
    if space == "w2":
        x = torch.cat([x, ls.exp()], dim=1).contiguous()
    n = x.shape[0]
    if queries is not None and (isinstance(queries, bool) or int(queries) != queries or not 1 <= int(queries) <= n):
        raise ValueError("%s: queries must be None or an integer in [1, n = %d]" % (what, n))
    queries = None if queries is None else int(queries)

    if method == "labels":
        res = _indices(what, x, label.contiguous(), classes, metric, queries, seed)
        res.update(method=method, space=space, k=classes)
        return res
    if method == "posterior":
        rows = []
        for image, _ in (data if chunk_rows is None else regroup(what, data, chunk_rows)):
            with torch.no_grad():
                rows.append(model.encode(image)[2].argmax(dim=1))      # log alpha (SHOT-VAE) or alpha (smooth): the same first maximum
        res = _indices(what, x, torch.cat(rows).long().contiguous(), classes, metric, queries, seed)
        res.update(method=method, space=space, k=classes)
        return res
    results = []
    for kk in ks:
        cluster = KMeans(kk, x.shape[1], seed=seed, **kmeans_args).fit(x, **fit_args).predict(x)
        res = _indices(what, x, cluster, kk, metric, queries, seed)
        res.update(method=method, space=space, k=kk)
        results.append(res)
    if not isinstance(k, (list, tuple)):
        return results[0]
    scores = [r["silhouette"] for r in results]
    best = max(range(len(ks)), key=lambda i: (scores[i] == scores[i], scores[i] if scores[i] == scores[i] else 0.0))
    return dict(results=results, ks=ks, best_k=ks[best])
