"""How good are the generated samples?  A set of generated rows against a set of real ones, on the HIP path (csrc/manifold.hip; DESIGN.md
4g): the Frechet distance of their feature distributions, improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage
(Naeem et al. 2020).

    real, fake = Manifold(128), Manifold(128)
    real.add(real_mu); fake.add(fake_mu)
    real.fit(5); fake.fit(5)                                            # the 5th-neighbour radius of every row
    inside = real.count(fake.mu)                                        # int64 [n_fake]: the real balls each fake row lies in

    manifold_metrics(real_mu, fake_mu, k=5)                             # precision, recall, density, coverage
    frechet_distance(moments_real, moments_fake)                        # two FeatureMoments
    evaluate_generation(model, loader)                                  # all of them, for the model's own samples

A radius is a value of LatentIndex.search's list: in the metric's own, SQUARED, units.  `ls` is LOG SIGMA everywhere.  The [queries,
gallery] matrix is never stored; nothing here synchronises with the host except where stated, and there is no CPU fallback."""
import numpy as np
import torch

from . import _lib as L
from .aggregate import partials
from ._latent import _p, _st, eval_only, latent_family, on_device, split_batch
from .neighbors import LatentIndex, MAX_K, encode_posterior, metric_code, posterior_rows

BALL_METRICS = (L.DIST_EUCLID, L.DIST_W2)
FIT_CHUNK = 8192              # query rows per search of fit(): the lists stay at FIT_CHUNK x k slots


def _ball_metric(what, metric):
    code = metric_code(metric)
    if code not in BALL_METRICS:
        raise ValueError("%s: a k-th-neighbour radius needs a symmetric distance (\"euclid\" or \"w2\"), not %r: KL is not symmetric and "
                         "the cosine is a similarity" % (what, metric))
    return code


class Manifold:
    """A device-resident set of rows (a LatentIndex's doubling buffers), each the centre of a ball that reaches to its k-th nearest
    neighbour in the set, and the membership counts sv_ball_scan takes over them.

    count() issues no host synchronisation and, once the set is fitted, can be captured under torch.cuda.graph and replayed on new
    queries."""

    def __init__(self, dim, metric="euclid"):
        self.code = _ball_metric("Manifold", metric)
        self.index = LatentIndex(dim, metric)
        self.dim, self.metric = self.index.dim, metric
        self.radii = self.k = None

    def __len__(self):
        return len(self.index)

    @property
    def mu(self):
        return self.index.mu[:len(self.index)]

    @property
    def ls(self):
        return None if self.index.ls is None else self.index.ls[:len(self.index)]

    def add(self, mu, ls=None):
        """appends the rows (mu, ls) [n, dim] (ls: "w2" only); returns the index of the first row added.  The radii of an earlier
        fit() no longer describe the set: fit again."""
        first = self.index.add(mu, ls)
        self.radii = self.k = None
        return first

    def fit(self, k):
        """sets the radius of every row to the distance of its k-th nearest OTHER row (leave-one-out; LatentIndex.search over the set
        itself, FIT_CHUNK queries at a time); -> radii fp32 [len]"""
        k, N = int(k), len(self.index)
        if not 1 <= k <= MAX_K:
            raise ValueError("k must be in [1, %d] (sv_knn_scan keeps four list slots per lane); got %d" % (MAX_K, k))
        if N <= k:
            raise ValueError("Manifold.fit: the k-th neighbour of a row needs more than k = %d rows; the set has %d" % (k, N))
        radii = torch.empty(N, dtype=torch.float32, device=self.index.mu.device)
        mu, ls = self.mu, self.ls
        for a in range(0, N, FIT_CHUNK):
            val = self.index.search(mu[a:a + FIT_CHUNK], None if ls is None else ls[a:a + FIT_CHUNK], k=k, exclude_self_from=a)[0]
            radii[a:a + FIT_CHUNK] = val[:, k - 1]
        self.radii, self.k = radii, k
        return radii

    def count(self, mu, ls=None, gallery_count=None, exclude_self_from=None):
        """-> int64 [Q]: the number of balls of the set that each query row lies in (value finite and <= the ball's radius).
        gallery_count (int64 [len], a caller-owned device tensor) is ADDED TO: [j] += the number of the queries inside ball j.
        exclude_self_from = s: query i is row s + i of the set and is not counted in its own ball."""
        if self.radii is None:
            raise ValueError("Manifold.count: the set has no radii (never fitted, or rows were added since): call fit(k) first")
        if torch.is_tensor(gallery_count) and not gallery_count.is_cuda:
            raise L.ShotVaeHipError("Manifold.count: gallery_count is not on an MI355X (no CPU fallback)")
        mu, ls = posterior_rows("Manifold.count", self.code, mu, ls, dim=self.dim)
        N, Q = len(self.index), mu.shape[0]
        if gallery_count is not None and (not torch.is_tensor(gallery_count) or gallery_count.dtype != torch.int64
                                          or tuple(gallery_count.shape) != (N,) or not gallery_count.is_contiguous()):
            raise ValueError("Manifold.count: gallery_count must be a contiguous int64 device tensor [%d]" % N)
        self_from = -1 if exclude_self_from is None else int(exclude_self_from)
        if self_from < -1:
            raise ValueError("exclude_self_from must be >= 0")
        out = torch.zeros(Q, dtype=torch.int64, device=mu.device)
        L.call("sv_ball_scan", self.code, _p(mu), _p(ls), Q, _p(self.index.mu), _p(self.index.ls), _p(self.radii), N, self.dim, 0,
               self_from, partials(-(-Q // 64), N), _p(out), _p(gallery_count), _st())
        return out


def _manifold_sums(real, fake):
    """the four integer sums behind the metrics, int64 [4] on the device: fake rows inside a real ball, real rows inside a fake ball,
    the memberships of the fake rows in real balls, real balls that hold a fake row -- two scans"""
    held = torch.zeros(len(real), dtype=torch.int64, device=real.mu.device)
    in_real = real.count(fake.mu, fake.ls, gallery_count=held)
    in_fake = fake.count(real.mu, real.ls)
    return torch.stack([(in_real > 0).sum(), (in_fake > 0).sum(), in_real.sum(), (held > 0).sum()])


def _metrics_of(sums, n_real, n_fake, k):
    s = [int(v) for v in sums]
    return dict(precision=s[0] / n_fake, recall=s[1] / n_real, density=s[2] / (k * n_fake), coverage=s[3] / n_real, n_real=n_real,
                n_fake=n_fake)


def manifold_metrics(real_mu, fake_mu, real_ls=None, fake_ls=None, k=5, metric="euclid"):
    """The k-nearest-neighbour manifold measures of a generated set against a real one (rows [n, D] on the device; ls: "w2" only):

        precision   the share of fake rows inside at least one real ball                                     (Kynkaanniemi et al. 2019)
        recall      the share of real rows inside at least one fake ball
        density     the memberships of the fake rows in real balls / (k n_fake); may exceed 1                 (Naeem et al. 2020)
        coverage    the share of real balls that hold at least one fake row
        n_real, n_fake

    A ball reaches from a row to its k-th nearest other row of its own set.  Two fits and two scans (coverage comes from the precision
    scan's per-ball counts); the one host read is at the end."""
    _ball_metric("manifold_metrics", metric)
    if not torch.is_tensor(real_mu) or not torch.is_tensor(fake_mu) or real_mu.dim() != 2 or fake_mu.dim() != 2 \
            or real_mu.shape[1] != fake_mu.shape[1] or real_mu.shape[1] < 1:
        raise ValueError("manifold_metrics: real_mu and fake_mu must be matrices [n, D] of one D")
    real, fake = Manifold(real_mu.shape[1], metric), Manifold(real_mu.shape[1], metric)
    real.add(real_mu, real_ls)
    fake.add(fake_mu, fake_ls)
    real.fit(k)
    fake.fit(k)
    return _metrics_of(_manifold_sums(real, fake).cpu().tolist(), len(real), len(fake), int(k))


class FeatureMoments:
    """Running mean and covariance of feature rows, float64 on the device.  The sums are taken of x - shift with shift = the mean of
    the first batch, fixed afterwards (the shifted-data form: the covariance is not a small difference of two large numbers however far
    the features lie from the origin).  add() does not synchronise with the host.  A cold path in float64 torch: one [D, D] update per
    batch beside an encoder pass."""

    def __init__(self, dim):
        self.dim = int(dim)
        if self.dim < 1:
            raise ValueError("FeatureMoments: dim must be >= 1")
        self.rows = 0                  # (host side: the batch sizes are shapes)
        self.shift = self.n = self.s1 = self.s2 = None

    def add(self, x):
        on_device("FeatureMoments.add", x)
        if not torch.is_tensor(x) or x.dim() != 2 or x.shape[0] < 1 or x.shape[1] != self.dim:
            raise ValueError("FeatureMoments.add: x must be a non-empty matrix [n, %d]" % self.dim)
        x = x.detach().double()
        if self.shift is None:
            self.shift = x.mean(dim=0)
            self.n = torch.zeros((), dtype=torch.float64, device=x.device)
            self.s1 = torch.zeros(self.dim, dtype=torch.float64, device=x.device)
            self.s2 = torch.zeros(self.dim, self.dim, dtype=torch.float64, device=x.device)
        c = x - self.shift
        self.n += x.shape[0]
        self.s1 += c.sum(dim=0)
        self.s2 += c.t() @ c
        self.rows += x.shape[0]

    def _need(self, rows):
        if self.rows < rows:
            raise ValueError("FeatureMoments: %d row(s) added, %d needed" % (self.rows, rows))

    def mean(self):
        """float64 [dim] on the device"""
        self._need(1)
        return self.shift + self.s1 / self.n

    def cov(self):
        """the unbiased covariance, float64 [dim, dim] on the device"""
        self._need(2)
        return (self.s2 - torch.outer(self.s1, self.s1) / self.n) / (self.n - 1.0)


def _clean_spectrum(w):
    """eigenvalues of a matrix that is positive semi-definite in exact arithmetic: the negative ones, and those within the rounding noise
    of the largest (len(w) eps max w -- the size eigh's own error has), are zero.  Without the floor a rank-deficient covariance (fewer
    rows than dimensions) would add sqrt(noise) ~ 1e-8 per missing rank to the trace of the root."""
    top = float(w.max()) if w.size else 0.0
    return np.where(w > len(w) * np.finfo(np.float64).eps * max(top, 0.0), w, 0.0)


def frechet_from_moments(m1, s1, m2, s2):
    """|m1 - m2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1^1/2 S2 S1^1/2) of float64 numpy moments: eigh of S1, eigvalsh of the symmetric
    product -- real symmetric problems only, no complex arithmetic"""
    m1, s1, m2, s2 = (np.asarray(a, dtype=np.float64) for a in (m1, s1, m2, s2))
    w, v = np.linalg.eigh(0.5 * (s1 + s1.T))
    root = (v * np.sqrt(_clean_spectrum(w))) @ v.T
    prod = root @ (0.5 * (s2 + s2.T)) @ root
    ev = _clean_spectrum(np.linalg.eigvalsh(0.5 * (prod + prod.T)))
    d = m1 - m2
    return float(d @ d + np.trace(s1) + np.trace(s2) - 2.0 * np.sqrt(ev).sum())


def frechet_distance(a, b):
    """The Frechet distance of the Gaussians fitted to two FeatureMoments (the FID's formula on whatever features they saw), in float64
    on the host after ONE copy of the two moment sets: the one synchronisation."""
    for t in (a, b):
        if not isinstance(t, FeatureMoments):
            raise TypeError("frechet_distance: two FeatureMoments, not %s" % type(t).__name__)
    a._need(2)
    b._need(2)
    if a.dim != b.dim:
        raise ValueError("frechet_distance: the moments have %d and %d dimensions" % (a.dim, b.dim))
    D = a.dim
    flat = torch.cat([a.mean(), a.cov().reshape(-1), b.mean().to(a.s1.device), b.cov().reshape(-1).to(a.s1.device)]).cpu().numpy()
    m1, s1, m2, s2 = flat[:D], flat[D:D + D * D].reshape(D, D), flat[D + D * D:2 * D + D * D], flat[2 * D + D * D:].reshape(D, D)
    return frechet_from_moments(m1, s1, m2, s2)


def evaluate_generation(model, batches, source="generate", space="mu", k=5, metric="euclid", key=0, tau=1.0, mixture=None):
    """The quality of what `model` (a VariationalAutoEncoder or a SmoothVAE, in eval mode: NotImplementedError otherwise, as for score)
    generates, against the images of `batches` ((image, label) or (image,) tuples, or image tensors, on the device).

        source  "generate"     as many class-conditional samples as there are images, with the data's labels in order (the predicted class
                               where a batch carries none), drawn with `key` and `tau` at row0 = the running index: the samples do not
                               depend on the batching
                "reconstruct"  the reconstructions of the same images (the reconstruction Frechet distance)
                "mixture"      as "generate", with the codes drawn from `mixture` (a fitted mixture.GaussianMixture) where "generate"
                               draws them from the prior: generate_from_mixture with `key` at row0 = the running index (`tau` is not read)
        space   "mu"           both sets are compared by their posterior means (encode_posterior; "w2" also reads log sigma)
                "features"     by the pooled encoder features (VariationalAutoEncoder only; "euclid" only: features have no sigma)

    The generated images go back into the encoder as the model emits them, so the real images must be in the range the model
    reconstructs.  -> frechet (FeatureMoments / frechet_distance over the rows), precision, recall, density, coverage (manifold_metrics'
    definitions with `k`, `metric`), n.  Two host reads at the end: the integer sums and the moments."""
    family = latent_family("evaluate_generation", model)
    if source not in ("generate", "reconstruct", "mixture"):
        raise ValueError("evaluate_generation: source must be 'generate', 'reconstruct' or 'mixture'")
    if (source == "mixture") != (mixture is not None):
        raise ValueError("evaluate_generation: source='mixture' needs a fitted mixture, and only that source takes one")
    if space not in ("mu", "features"):
        raise ValueError("evaluate_generation: space must be 'mu' or 'features'")
    code = _ball_metric("evaluate_generation", metric)
    if space == "features":
        if family != "shot":
            raise ValueError("evaluate_generation: space='features' needs a VariationalAutoEncoder (a SmoothVAE has no pooled features)")
        if code != L.DIST_EUCLID:
            raise ValueError("evaluate_generation: space='features' has no sigma: metric must be 'euclid'")
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError("evaluate_generation: k must be in [1, %d]" % MAX_K)
    if key is None:
        raise ValueError("evaluate_generation: the samples need a key")
    eval_only("evaluate_generation", model)

    def rows_of(image):
        if space == "features":
            return model.features(image).float().contiguous(), None
        mu, ls = encode_posterior(model, image)
        return mu, (ls if code == L.DIST_W2 else None)

    real = fake = mom_real = mom_fake = None
    count = 0
    for batch in batches:
        image, label = split_batch("evaluate_generation", batch, False)
        if source in ("generate", "mixture"):
            if label is None:
                label = model.predict(image)
            if source == "mixture":
                from .mixture import generate_from_mixture
                made = generate_from_mixture(model, mixture, label, key, row0=count)
            else:
                made = model.generate(label, key, tau=tau, row0=count)
        else:
            made = model.reconstruct(image)
        r_mu, r_ls = rows_of(image)
        f_mu, f_ls = rows_of(made)
        if real is None:
            D = r_mu.shape[1]
            real, fake, mom_real, mom_fake = Manifold(D, metric), Manifold(D, metric), FeatureMoments(D), FeatureMoments(D)
        real.add(r_mu, r_ls)
        fake.add(f_mu, f_ls)
        mom_real.add(r_mu)
        mom_fake.add(f_mu)
        count += image.shape[0]
    if real is None:
        raise ValueError("evaluate_generation: the dataset is empty")
    real.fit(k)
    fake.fit(k)
    res = _metrics_of(_manifold_sums(real, fake).cpu().tolist(), count, count, k)
    del res["n_real"], res["n_fake"]
    res.update(frechet=frechet_distance(mom_real, mom_fake), n=count)
    return res
