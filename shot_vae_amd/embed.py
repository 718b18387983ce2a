"""The picture of the latent space: a 2-D (or 3-D) t-SNE map of the posteriors, on the HIP path (csrc/tsne.hip).

    ts = TSNE(perplexity=30.0, metric="kl").fit(mu, ls)                # van der Maaten & Hinton 2008; scikit-learn 1.7's defaults
    ts.embedding_, ts.kl_divergence_, ts.n_iter_                       # fp32 [N, 2] on the device, float, int
    evaluate_embedding(model, loader)                                  # embedding, labels, neighbourhood_hit, neighbourhood_preservation

The input side is LatentIndex.search (the k nearest posteriors under "kl" / "w2" / "euclid", the value used as is; "cosine" holds
similarities and is refused) and sv_tsne_affinity; an iteration is sv_tsne_attract, sv_tsne_repulse, sv_tsne_update: the EXACT gradient,
an all-pairs scan that never stores the [N, N] matrix.  No float atomic anywhere -- the same call sequence gives the same bits --,
step() does not synchronise with the host and can be captured, and there is no CPU fallback."""
import torch

from . import _lib as L
from .aggregate import partials
from ._latent import _p, _st, eval_only, gather_codes, latent_family, num_classes, on_device, take_args
from .neighbors import MAX_K, LatentIndex

REPULSE_ROWS = 256            # sv_tsne_repulse: rows per block


def repulse_partials(n):
    """P of sv_tsne_repulse for n points: aggregate.partials' rule over its grid of ceil(n / 256) blocks per state.  A function of the
    shape alone."""
    return partials(-(-n // REPULSE_ROWS), n)


def update_scratch(n):
    """the number of doubles sv_tsne_update needs as scratch for n points"""
    return 3 * (-(-n // 256))


def conditional_affinities(dist, idx, perplexity, tol=1e-5, max_steps=100):
    """The conditional affinities p_j|i of every row's k-list (dist fp32 [N, k], idx int64 [N, k], closest first, as LatentIndex.search
    returns them): p_j|i = exp(-beta_i (d_ij - d_i,min)) / sum over the valid slots (idx >= 0 and a finite dist; p = 0 on the others),
    beta_i by scikit-learn's bisection in double until |H_i - log(perplexity)| <= tol or max_steps evaluations (sv_tsne_affinity).
    -> (p fp32 [N, k], beta float64 [N], steps int32 [N]; steps == max_steps: the tolerance was not met, or the row has fewer than two
    valid slots and is uniform over what it has)"""
    if not torch.is_tensor(dist) or not torch.is_tensor(idx) or dist.dim() != 2 or tuple(idx.shape) != tuple(dist.shape) \
            or idx.dtype != torch.int64 or dist.shape[0] < 1:
        raise ValueError("conditional_affinities: dist [N, k] and idx int64 [N, k] of one shape")
    n, k = dist.shape
    perplexity, tol, max_steps = float(perplexity), float(tol), int(max_steps)
    if not 1 <= k <= MAX_K:
        raise ValueError("conditional_affinities: k must be in [1, %d]; got %d" % (MAX_K, k))
    if not 1.0 < perplexity < k:
        raise ValueError("conditional_affinities: perplexity must be in (1, k = %d); got %g" % (k, perplexity))
    if tol < 0 or max_steps < 1:
        raise ValueError("conditional_affinities: tol >= 0 and max_steps >= 1")
    on_device("conditional_affinities", dist, idx)
    dist, idx = dist.detach().float().contiguous(), idx.contiguous()
    p = torch.empty_like(dist)
    beta = torch.empty(n, dtype=torch.float64, device=dist.device)
    steps = torch.empty(n, dtype=torch.int32, device=dist.device)
    L.call("sv_tsne_affinity", _p(dist), _p(idx), n, k, perplexity, tol, max_steps, _p(p), _p(beta), _p(steps), _st())
    return p, beta, steps


def symmetrize(p, idx):
    """The joint P = (P_cond + P_cond^T) / (2N) over the union of the edges, as CSR: -> (rowptr int64 [N + 1], col int64 [nnz], val
    fp32 [nnz]), the columns of a row ascending; the values sum to 1 when every row of p does.  p [N, k] on the lists idx [N, k]; a
    slot with idx < 0 or p <= 0 is no edge.  Plain torch, once per fit: both directions of every edge, a stable sort by row * N + col,
    and the runs merged -- a cell receives at most two addends (the lists of LatentIndex.search hold a gallery row once), so its sum
    does not depend on their order; there is no index_add_ on floats."""
    if not torch.is_tensor(p) or not torch.is_tensor(idx) or p.dim() != 2 or tuple(p.shape) != tuple(idx.shape) or idx.dtype != torch.int64:
        raise ValueError("symmetrize: p [N, k] and idx int64 [N, k] of one shape")
    n, k = p.shape
    dev = p.device
    row = torch.arange(n, device=dev).repeat_interleave(k)
    col, v = idx.reshape(-1), p.reshape(-1).double()
    keep = (col >= 0) & (col < n) & (v > 0)
    row, col, v = row[keep], col[keep], v[keep]
    key = torch.cat([row * n + col, col * n + row])
    key, order = torch.sort(key, stable=True)
    v = torch.cat([v, v])[order]
    cell, count = torch.unique_consecutive(key, return_counts=True)
    first = torch.cumsum(count, 0) - count
    second = v[torch.clamp(first + 1, max=max(v.numel() - 1, 0))] if v.numel() else v
    val = (v[first] + torch.where(count > 1, second, torch.zeros_like(second))) / (2.0 * n)
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    rowptr[1:] = torch.cumsum(torch.bincount(cell // n, minlength=n), 0)
    return rowptr, (cell % n).contiguous(), val.float().contiguous()


def pca_project(x, d):
    """scikit-learn's PCA initialisation in float64: the rows of x about their mean on the top d eigenvectors of the covariance
    (torch.linalg.eigh), every vector signed so that its largest-magnitude entry is positive, the whole scaled so that the first column
    has (population) standard deviation 1e-4.  -> float64 [N, d] on x's device"""
    if not torch.is_tensor(x) or x.dim() != 2 or x.shape[0] < 2 or not 1 <= int(d) <= x.shape[1]:
        raise ValueError("pca_project: x [N >= 2, D] and 1 <= d <= D")
    x = x.detach().double()
    xc = x - x.mean(dim=0, keepdim=True)
    cov = xc.t() @ xc / (x.shape[0] - 1)
    _, vec = torch.linalg.eigh(cov)                    # ascending eigenvalues
    vec = vec[:, -int(d):].flip(1)
    big = vec.abs().argmax(dim=0)
    vec = vec * torch.sign(vec[big, torch.arange(vec.shape[1], device=vec.device)])
    y = xc @ vec
    return y / y[:, 0].std(unbiased=False) * 1e-4


class TSNE:
    """Exact t-SNE of N posteriors into n_components in {2, 3} dimensions.

    k neighbours per row enter the affinities (default min(int(3 perplexity), N - 1, 256)); learning_rate "auto" is
    max(N / early_exaggeration / 4, 50); init is "pca" (pca_project of the means), "random" (1e-4 x normal draws of a
    torch.Generator seeded with `seed`) or a device tensor [N, n_components].  The first exaggeration_iter iterations run with
    P x early_exaggeration and momentum 0.5, the rest with P and momentum 0.8.

    prepare() builds the index, the k-lists, the CSR form of P and the state; step() is one iteration -- sv_tsne_attract,
    sv_tsne_repulse, sv_tsne_update on buffers that prepare() allocated --, issues no host synchronisation and can be captured under
    torch.cuda.graph; the schedule lives in the device vector `hyper` (exaggeration, momentum, learning rate), which set_phase()
    rewrites by a device copy: one captured graph serves both phases.  After fit(): embedding_ (fp32 [N, n_components] on the device),
    kl_divergence_ (the KL at the start of the last iteration) and n_iter_."""

    def __init__(self, n_components=2, perplexity=30.0, k=None, metric="euclid", early_exaggeration=12.0, exaggeration_iter=250,
                 learning_rate="auto", n_iter=1000, init="pca", seed=0):
        self.n_components, self.perplexity, self.metric = int(n_components), float(perplexity), metric
        if self.n_components not in (2, 3):
            raise ValueError("TSNE: n_components must be 2 or 3")
        if metric not in ("kl", "w2", "wasserstein", "euclid", "euclidean"):
            raise ValueError("TSNE: metric must be 'kl', 'w2' or 'euclid' ('cosine' holds similarities, not distances); got %r" % (metric,))
        if not self.perplexity > 1.0:
            raise ValueError("TSNE: perplexity must be > 1")
        self.k = None if k is None else int(k)
        if self.k is not None:
            if not 1 <= self.k <= MAX_K:
                raise ValueError("TSNE: k must be in [1, %d]; got %d" % (MAX_K, self.k))
            if self.perplexity >= self.k:
                raise ValueError("TSNE: perplexity = %g must be below k = %d" % (self.perplexity, self.k))
        self.early_exaggeration, self.exaggeration_iter = float(early_exaggeration), int(exaggeration_iter)
        self.n_iter, self.seed = int(n_iter), int(seed)
        if self.n_iter < 1 or self.exaggeration_iter < 0 or not self.early_exaggeration > 0:
            raise ValueError("TSNE: n_iter >= 1, exaggeration_iter >= 0 and early_exaggeration > 0")
        if learning_rate != "auto" and not float(learning_rate) > 0:
            raise ValueError("TSNE: learning_rate must be 'auto' or > 0")
        self.learning_rate = learning_rate
        if torch.is_tensor(init):
            if init.dim() != 2 or init.shape[1] != self.n_components:
                raise ValueError("TSNE: init must be a tensor [N, %d]" % self.n_components)
            on_device("TSNE", init)
        elif init not in ("pca", "random"):
            raise ValueError("TSNE: init must be 'pca', 'random' or a tensor [N, n_components]")
        self.init = init
        self.embedding_ = self.kl_divergence_ = None
        self.n_iter_ = 0
        self.y = None

    def prepare(self, mu, ls=None):
        """the k-lists of the posteriors (mu, ls) [N, dim] under the metric (ls: log sigma, None for "euclid"), their affinities, the
        CSR form of P, the initial embedding and every buffer step() touches; leaves the early phase set"""
        if not torch.is_tensor(mu) or mu.dim() != 2 or mu.shape[0] < 2:
            raise ValueError("TSNE: mu must be a matrix [N >= 2, dim]")
        n, d = mu.shape[0], self.n_components
        k = self.k if self.k is not None else min(int(3 * self.perplexity), n - 1, MAX_K)
        if k < 1 or self.perplexity >= k:
            raise ValueError("TSNE: perplexity = %g must be below k = %d (N = %d)" % (self.perplexity, k, n))
        if torch.is_tensor(self.init) and self.init.shape[0] != n:
            raise ValueError("TSNE: init has %d rows, the data %d" % (self.init.shape[0], n))
        on_device("TSNE", mu, ls)
        dev = mu.device
        index = LatentIndex(mu.shape[1], self.metric)
        index.add(mu, ls)
        self.knn_dist, self.knn_idx = index.search(mu, ls, k=k, exclude_self_from=0)
        self.p_cond, self.beta, self.search_steps = conditional_affinities(self.knn_dist, self.knn_idx, self.perplexity)
        self.rowptr, self.col, self.val = symmetrize(self.p_cond, self.knn_idx)

        if torch.is_tensor(self.init):
            y = self.init.detach().float()
        elif self.init == "pca":
            y = pca_project(mu, d).float()
        else:
            gen = torch.Generator().manual_seed(self.seed)
            y = (1e-4 * torch.randn(n, d, dtype=torch.float32, generator=gen)).to(dev)
        self.n, self.k_used, self.P = n, k, repulse_partials(n)
        self.y = y.contiguous().clone()
        self.vel, self.gain = torch.zeros_like(self.y), torch.ones_like(self.y)
        self.attr = torch.empty(n, d, dtype=torch.float32, device=dev)
        self.rowkl = torch.empty(n, dtype=torch.float32, device=dev)
        self.rep = torch.empty(self.P, n, d, dtype=torch.float32, device=dev)
        self.z = torch.empty(self.P, n, dtype=torch.float32, device=dev)
        self.scratch = torch.empty(update_scratch(n), dtype=torch.float64, device=dev)
        self.stats = torch.zeros(3, dtype=torch.float32, device=dev)
        lr = max(n / self.early_exaggeration / 4.0, 50.0) if self.learning_rate == "auto" else float(self.learning_rate)
        self.lr = lr
        self._phases = (torch.tensor([self.early_exaggeration, 0.5, lr], dtype=torch.float32).to(dev),
                        torch.tensor([1.0, 0.8, lr], dtype=torch.float32).to(dev))
        self.hyper = self._phases[0].clone()
        self.n_iter_ = 0
        return self

    def set_phase(self, late):
        """writes `hyper` for the early (exaggerated, momentum 0.5) or the late (momentum 0.8) phase: a device copy, no new arguments"""
        self.hyper.copy_(self._phases[1 if late else 0])

    def step(self):
        """one iteration in place -> stats fp32 [3] on the device: the KL and Z at the embedding the step STARTED from, and |g|^2"""
        if self.y is None:
            raise ValueError("TSNE.step: call prepare() or fit() first")
        n, d = self.n, self.n_components
        L.call("sv_tsne_attract", _p(self.y), n, d, _p(self.rowptr), _p(self.col), _p(self.val), _p(self.attr), _p(self.rowkl), _st())
        L.call("sv_tsne_repulse", _p(self.y), n, d, self.P, _p(self.rep), _p(self.z), _st())
        L.call("sv_tsne_update", _p(self.y), _p(self.vel), _p(self.gain), _p(self.attr), _p(self.rowkl), _p(self.rep), _p(self.z), self.P, n,
               d, _p(self.hyper), _p(self.scratch), _p(self.stats), _st())
        return self.stats

    def fit(self, mu, ls=None, check_every=50, min_grad_norm=1e-7):
        """prepare() and up to n_iter iterations.  `stats` is read on the host once per check_every iterations of the late phase (None:
        never; exactly n_iter iterations) and the run ends when the gradient norm is <= min_grad_norm, scikit-learn's rule."""
        if check_every is not None and int(check_every) < 1:
            raise ValueError("TSNE.fit: check_every must be >= 1 or None")
        self.prepare(mu, ls)
        for it in range(self.n_iter):
            if it == self.exaggeration_iter:
                self.set_phase(True)
            self.step()
            self.n_iter_ = it + 1
            if check_every is not None and it >= self.exaggeration_iter and (it + 1) % int(check_every) == 0:
                if float(self.stats.cpu()[2]) ** 0.5 <= min_grad_norm:
                    break
        self.embedding_ = self.y
        self.kl_divergence_ = float(self.stats.cpu()[0])
        return self


def neighbourhood_preservation(idx_a, idx_b, chunk=4096):
    """the mean over the rows of the share of a row's neighbours in idx_a [N, k] found among its neighbours in idx_b [N, k] (entries
    < 0 are no neighbours) -> a 0-dim float64 tensor on the lists' device; plain torch"""
    if idx_a.shape != idx_b.shape or idx_a.dim() != 2:
        raise ValueError("neighbourhood_preservation: two lists [N, k] of one shape")
    total = torch.zeros((), dtype=torch.float64, device=idx_a.device)
    for lo in range(0, idx_a.shape[0], chunk):
        a, b = idx_a[lo:lo + chunk], idx_b[lo:lo + chunk]
        found = ((a[:, :, None] == b[:, None, :]).any(dim=2) & (a >= 0)).sum(dim=1)
        total += (found.double() / idx_a.shape[1]).sum()
    return total / idx_a.shape[0]


def evaluate_embedding(model, data, k=10, chunk_rows=256, **tsne_args):
    """The t-SNE map of the posteriors of `data` ((image, label) batches on the device) under `model` (a VariationalAutoEncoder or a
    SmoothVAE, in eval mode: NotImplementedError otherwise, as for evaluate_clustering), and how well it keeps the classes and the
    neighbourhoods.  tsne_args: TSNE's arguments, and fit's check_every / min_grad_norm.  The images are regrouped into batches of
    chunk_rows rows before the model sees them (the encoders' last bits depend on the batch size, and t-SNE's trajectories are chaotic),
    and the rows are gathered before anything is embedded: the result does not depend on how the caller batched the set, only on the
    order of its rows.  chunk_rows=None takes the batches as they come.  ->

        embedding                   fp32 [N, n_components] on the device, in the order of the data
        labels                      int64 [N] on the device
        kl, n_iter                  TSNE's kl_divergence_ and n_iter_
        neighbourhood_hit           the leave-one-out k-NN label accuracy IN THE EMBEDDING (LatentIndex("euclid"), sv_knn_vote)
        neighbourhood_preservation  the mean share of a row's k latent neighbours (TSNE's metric) found among its k embedded neighbours"""
    latent_family("evaluate_embedding", model)
    eval_only("evaluate_embedding", model)
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError("evaluate_embedding: k must be in [1, %d]" % MAX_K)
    if chunk_rows is not None and int(chunk_rows) < 1:
        raise ValueError("evaluate_embedding: chunk_rows must be >= 1 or None")
    fit_args = take_args(tsne_args, ("check_every", "min_grad_norm"))
    ts = TSNE(**tsne_args)

    classes = num_classes(model)
    mu, ls, label = gather_codes("evaluate_embedding", model, data, chunk_rows=chunk_rows)
    n = mu.shape[0]
    if k > n - 1:
        raise ValueError("evaluate_embedding: k = %d neighbours from %d rows" % (k, n))
    ts.fit(mu, ls, **fit_args)

    y = ts.embedding_
    emb = LatentIndex(ts.n_components, "euclid", num_classes=classes)
    emb.add(y, None, label)
    val, idx = emb.search(y, None, k=k, exclude_self_from=0)
    pred = torch.empty(n, dtype=torch.int64, device=y.device)
    counts = torch.zeros(2, dtype=torch.int64, device=y.device)
    L.call("sv_knn_vote", _p(val), _p(idx), n, k, _p(emb.labels), n, classes, 0, 1.0, _p(label.contiguous()), _p(pred), None, _p(counts),
           None, _st())
    lat = LatentIndex(mu.shape[1], ts.metric)
    lat.add(mu, ls)
    lat_idx = lat.search(mu, ls, k=k, exclude_self_from=0)[1]
    host = torch.cat([counts.double(), neighbourhood_preservation(lat_idx, idx).reshape(1)]).cpu()
    return dict(embedding=y, labels=label, kl=ts.kl_divergence_, n_iter=ts.n_iter_, neighbourhood_hit=float(host[0] / host[1]),
                neighbourhood_preservation=float(host[2]))
