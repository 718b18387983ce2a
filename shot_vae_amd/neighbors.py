"""Comparing one image's posterior with another's: pairwise distance matrices (lib/utils/calculate_dist.py of the reference) and
k-nearest-neighbour search / classification in latent space, on the HIP path (csrc/knn.hip).

    from shot_vae_amd.neighbors import pairwise_norm_kl_dist_gpu        # replaces `from lib.utils.calculate_dist import ...`

    index = LatentIndex(128, metric="kl", num_classes=10)
    for image, label in labelled_loader:
        index.add(*encode_posterior(model, image), label)
    dist, idx = index.search(*encode_posterior(model, query), k=20)      # nearest gallery rows, closest first
    pred = index.classify(*encode_posterior(model, query), k=20)         # k-NN vote

`ls` is LOG SIGMA everywhere (the SHOT-VAE convention; encode_posterior halves a smooth model's logvar).  The fused search never
stores the [queries, gallery] matrix; nothing here synchronises with the host, and there is no CPU fallback."""
import torch

from . import _lib as L
from ._latent import _p, _st, eval_only, latent_family, on_device

METRICS = {"kl": L.DIST_KL, "w2": L.DIST_W2, "wasserstein": L.DIST_W2, "euclid": L.DIST_EUCLID, "euclidean": L.DIST_EUCLID,
           "cosine": L.DIST_COSINE}
MAX_K = 256


def metric_code(metric):
    if metric not in METRICS:
        raise ValueError("unknown metric %r (one of %s)" % (metric, ", ".join(sorted(METRICS))))
    return METRICS[metric]


def _reads_ls(code):
    return code in (L.DIST_KL, L.DIST_W2)


def posterior_rows(what, code, mu, ls, dim=None):
    """(mu, ls) as contiguous fp32 device matrices [n, d]; ls = None where the metric does not read it"""
    on_device(what, mu, ls)
    if not torch.is_tensor(mu) or mu.dim() != 2 or mu.shape[0] < 1 or mu.shape[1] < 1:
        raise ValueError("%s: mu must be a non-empty matrix [n, d]" % what)
    if dim is not None and mu.shape[1] != dim:
        raise ValueError("%s: mu has %d columns, the index %d" % (what, mu.shape[1], dim))
    mu = mu.detach().float().contiguous()
    if not _reads_ls(code):
        return mu, None
    if not torch.is_tensor(ls) or tuple(ls.shape) != tuple(mu.shape):
        raise ValueError("%s: this metric reads log sigma: ls must have mu's shape %s" % (what, list(mu.shape)))
    return mu, ls.detach().float().contiguous()


def pairwise_distance(mu1, ls1, mu2, ls2=None, metric="kl"):
    """The [n1, n2] fp32 matrix of `metric` between the posteriors (mu1, ls1) and (mu2, ls2), the first argument first:
    "kl" KL(N_1 || N_2), "w2" the squared 2-Wasserstein distance, "euclid" the squared distance of the means, "cosine" the reference's
    mu1 . mu2 / (|mu1|^2 |mu2|^2) (a similarity).  The last two ignore ls (pass None)."""
    code = metric_code(metric)
    mu1, ls1 = posterior_rows("pairwise_distance", code, mu1, ls1)
    mu2, ls2 = posterior_rows("pairwise_distance", code, mu2, ls2, dim=mu1.shape[1])
    out = torch.empty(mu1.shape[0], mu2.shape[0], dtype=torch.float32, device=mu1.device)
    L.call("sv_pairdist", code, _p(mu1), _p(ls1), mu1.shape[0], _p(mu2), _p(ls2), mu2.shape[0], mu1.shape[1], _p(out), out.shape[1],
           _st())
    return out


# ---- the reference's names (lib/utils/calculate_dist.py): same argument orders, same results ----
def pairwise_norm_kl_dist_gpu(u1, log_sigma1, u2, log_sigma2):
    """[i, j] = KL((u1[i], log_sigma1[i]) || (u2[j], log_sigma2[j]))"""
    return pairwise_distance(u1, log_sigma1, u2, log_sigma2, "kl")


def pairwise_square_euclidean_gpu(v1, v2):
    return pairwise_distance(v1, None, v2, None, "euclid")


def pairwise_norm_wasserstein_dist_gpu(u1, log_sigma1, u2, log_sigma2):
    return pairwise_distance(u1, log_sigma1, u2, log_sigma2, "w2")


def calculate_mean_dist_pairwise(u1, u2, GPU_flag=True, distance="euclidean"):
    """the reference's signature; tensors (or numpy arrays) must be on the device's side of it: GPU_flag=False -- the reference's numpy
    path -- is refused like any other CPU input"""
    if distance not in ("euclidean", "cosine"):
        raise NotImplementedError("distance {} not implemented".format(distance))
    if not GPU_flag:
        raise L.ShotVaeHipError("calculate_mean_dist_pairwise: GPU_flag=False asks for the CPU path; there is no CPU fallback")
    u1, u2 = (torch.from_numpy(u).float().cuda() if not torch.is_tensor(u) else u for u in (u1, u2))
    return pairwise_distance(u1, None, u2, None, "euclid" if distance == "euclidean" else "cosine")


def encode_posterior(model, x):
    """(mu, log_sigma), fp32 [B, d] each, of the images x under `model`: a VariationalAutoEncoder's encode(), or a SmoothVAE's
    encode() with log_sigma = logvar / 2.  Eval mode only, as every inference call; no gradients."""
    if latent_family("encode_posterior", model) == "shot":
        mu, ls = model.encode(x)[:2]
        return mu.float().contiguous(), ls.float().contiguous()
    eval_only("encode_posterior", model)
    on_device("encode_posterior", x)
    with torch.no_grad():
        mean, logvar = model.encode(x)[:2]
        return mean.float().contiguous(), (0.5 * logvar.float()).contiguous()


class LatentIndex:
    """A device-resident gallery of posteriors and (optionally) labels, searched by sv_knn_scan.

    add() appends rows; the buffers grow by doubling, so n rows added in any number of calls are copied O(n) times in total and the
    rows already stored are not touched by an add that fits.  search() / classify() read the first len(index) rows; they issue no host
    synchronisation and, once the gallery is fixed, can be captured under torch.cuda.graph and replayed on new queries."""

    def __init__(self, dim, metric="kl", num_classes=None):
        self.dim, self.metric, self.code = int(dim), metric, metric_code(metric)
        if self.dim < 1:
            raise ValueError("LatentIndex: dim must be >= 1")
        self.num_classes = None if num_classes is None else int(num_classes)
        self.mu = self.ls = self.labels = None
        self.n = 0

    def __len__(self):
        return self.n

    def _grow(self, need, device):
        cap = 0 if self.mu is None else self.mu.shape[0]
        if need <= cap:
            return
        new = max(need, 2 * cap, 1024)
        for name, shape, dt in (("mu", (new, self.dim), torch.float32), ("ls", (new, self.dim), torch.float32),
                                ("labels", (new,), torch.int64)):
            if name == "ls" and not _reads_ls(self.code):
                continue
            buf = torch.empty(shape, dtype=dt, device=device)
            old = getattr(self, name)
            if old is not None:
                buf[:self.n] = old[:self.n]
            setattr(self, name, buf)

    def add(self, mu, ls=None, labels=None):
        """appends the rows (mu, ls) [n, dim] (ls may be None for "euclid" / "cosine") with their int64 labels [n] (None: unlabelled,
        such rows are found by search and cast no vote in classify); returns the global index of the first row added"""
        mu, ls = posterior_rows("LatentIndex.add", self.code, mu, ls, dim=self.dim)
        n = mu.shape[0]
        if labels is not None:
            if not torch.is_tensor(labels) or labels.numel() != n:
                raise ValueError("LatentIndex.add: labels must be a vector [%d]" % n)
            if not labels.is_cuda:
                raise L.ShotVaeHipError("LatentIndex.add: labels are not on an MI355X (no CPU fallback)")
        self._grow(self.n + n, mu.device)
        first = self.n
        self.mu[first:first + n] = mu
        if ls is not None:
            self.ls[first:first + n] = ls
        self.labels[first:first + n] = labels.reshape(-1).long() if labels is not None else -1
        self.n += n
        return first

    def _check_k(self, k):
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError("k must be in [1, %d] (sv_knn_scan keeps four list slots per lane); got %d" % (MAX_K, k))
        return k

    def search(self, mu, ls=None, k=1, exclude_self_from=None):
        """-> (dist [Q, k] fp32, idx [Q, k] int64): the k closest gallery rows of every query, closest first, ties by the smaller
        index; slots beyond the gallery's size are idx = -1, dist = +inf (-inf under "cosine", whose values are similarities).
        exclude_self_from = s: query i is gallery row s + i and is left out of its own list (leave-one-out)."""
        k = self._check_k(k)
        mu, ls = posterior_rows("LatentIndex.search", self.code, mu, ls, dim=self.dim)
        if self.n == 0:
            raise ValueError("LatentIndex.search: the index is empty")
        Q = mu.shape[0]
        val = torch.empty(Q, k, dtype=torch.float32, device=mu.device)
        idx = torch.empty(Q, k, dtype=torch.int64, device=mu.device)
        self_from = -1 if exclude_self_from is None else int(exclude_self_from)
        if self_from < -1:
            raise ValueError("exclude_self_from must be >= 0")
        L.call("sv_knn_scan", self.code, _p(mu), _p(ls), Q, _p(self.mu), _p(self.ls), self.n, self.dim, 0, self_from, k, _p(val),
               _p(idx), 1, _st())
        return val, idx

    def classify(self, mu, ls=None, k=1, weights="uniform", tau=1.0, label=None, counts=None, confusion=None, return_votes=False):
        """-> pred int64 [Q]: the class with the most votes among the k nearest labelled gallery rows (the first maximum; -1 when no
        neighbour voted).  weights="uniform": one vote each; "distance": exp(-dist / tau) (exp(similarity / tau) under "cosine").
        With `label` (int64 [Q]) the caller's device counters are ADDED to: counts int64 [2] += (hits, Q), confusion int64 [K, K]
        [label][pred] += 1 (the rules of SmoothVAE.classify).  return_votes: -> (pred, votes fp32 [Q, K])."""
        if weights not in ("uniform", "distance"):
            raise ValueError("weights must be 'uniform' or 'distance'")
        if self.num_classes is None:
            raise ValueError("LatentIndex.classify: the index was built without num_classes")
        K = self.num_classes
        on_device("LatentIndex.classify", label, counts, confusion)
        val, idx = self.search(mu, ls, k)
        Q = val.shape[0]
        if label is not None:
            if label.dtype != torch.int64 or label.numel() != Q:
                raise ValueError("classify: label must be an int64 vector [%d]" % Q)
            label = label.reshape(-1).contiguous()
        elif counts is not None or confusion is not None:
            raise ValueError("classify: counts / confusion need the labels")
        for t, shape, name in ((counts, (2,), "counts"), (confusion, (K, K), "confusion")):
            if t is not None and (t.dtype != torch.int64 or tuple(t.shape) != shape or not t.is_contiguous()):
                raise ValueError("classify: %s must be a contiguous int64 device tensor %s" % (name, list(shape)))
        mode = 0 if weights == "uniform" else (2 if self.code == L.DIST_COSINE else 1)
        pred = torch.empty(Q, dtype=torch.int64, device=val.device)
        votes = torch.empty(Q, K, dtype=torch.float32, device=val.device) if return_votes else None
        L.call("sv_knn_vote", _p(val), _p(idx), Q, val.shape[1], _p(self.labels), self.n, K, mode, float(tau), _p(label), _p(pred),
               _p(votes), _p(counts), _p(confusion), _st())
        return (pred, votes) if return_votes else pred
