"""A parametric density of the codes: diagonal Gaussian mixtures on the latent space, fitted by fused EM on the HIP path
(csrc/mixture.hip).

    gm = GaussianMixture(10, 128, seed=0).fit(mu)                      # k-means start, EM until the bound moves by < tol
    gm.score_samples(mu)                                               # log p(mu_i) under the mixture, fp32 [n] on the device
    gm.predict(mu), gm.predict_proba(mu)                               # the first maximum, the responsibilities
    gm.bic(mu), gm.aic(mu)                                             # to choose k
    z = gm.sample(64, key=0)                                           # "ex-post density estimation": codes to decode
    evaluate_mixture(model, loader, test_batches=test_loader, k=10)    # likelihoods against the prior, BIC / AIC, partition metrics
    generate_from_mixture(model, gm, labels, key=0)                    # images of mixture codes

Diagonal covariances only.  Rows must be finite: a NaN or infinite row has log-density NaN, is assigned to no component (-1) and enters
no parameter.  The [rows, components] matrix exists only where predict_proba asks for it, there is no atomic of any kind -- the same call
sequence gives the same bits --, nothing here synchronises with the host except where stated, and there is no CPU fallback."""
import math

import torch

from . import _lib as L
from .aggregate import partials
from ._latent import _p, _st, eval_only, gather_codes, latent_family, matrix, num_classes, on_device, resident_partials, take_args
from .cluster import KMeans, _partials as _kmeans_partials, contingency, partition_metrics

MAX_DIM = 1 << 20             # sv_gmm_accum: a block owns 32 dimensions, the grid's second dimension holds 65535 blocks
SLICE = 32
BLOCKS_PER_CU = 2             # sv_gmm_accum's blocks resident per compute unit (its launch bound)
KMEANS_STEPS = 10             # Lloyd steps behind the k-means++ seeding of init="kmeans"


def n_parameters(k, dim):
    """the free parameters of a diagonal mixture: k - 1 weights, k dim means, k dim variances"""
    return int(k) - 1 + 2 * int(k) * int(dim)


def _partials(k, dim, n):
    """P of sv_gmm_accum for n rows: aggregate.partials' rule over its grid of ceil(k / tile) x ceil(dim / 32) blocks per state (tile = 16
    components for k <= 16, else 64), lowered until the grid is resident at once (resident_partials).  A function of the shapes alone."""
    blocks = (1 if k <= 16 else -(-k // 64)) * -(-dim // SLICE)
    return resident_partials(partials(blocks, n), blocks, BLOCKS_PER_CU)


def _matrix(what, x, dim=None, k=None):
    """_latent.matrix for the mixture; k: that many components are to be seeded from the rows"""
    def limit(n):
        if k is not None and k > n:
            raise ValueError("%s: k = %d components from %d rows (k > N)" % (what, k, n))
    return matrix(what, x, dim, "the mixture", limit)


def _key_tensor(what, key, device):
    if torch.is_tensor(key):
        if key.dtype != torch.int64 or key.numel() != 1:
            raise ValueError("%s: key must be an int or a 1-element int64 device tensor" % what)
        if not key.is_cuda:
            raise L.ShotVaeHipError("%s: key is not on an MI355X (no CPU fallback)" % what)
        return key.reshape(1)
    if key is None or isinstance(key, bool):
        raise ValueError("%s: key must be an int or a 1-element int64 device tensor" % what)
    return torch.tensor([int(key)], dtype=torch.int64, device=device)


def _em_loop(step, read, max_iter, tol, check_every):
    """The iterations of one EM run and scikit-learn's stopping rule.  step() runs one iteration and returns a handle of its lower bound;
    read(previous, current) brings two handles' bounds to the host as floats (previous is None at the first iteration: its bound is
    -inf).  The bounds are read once per `check_every` iterations and at the last one; the run has converged when the bound of an
    iteration differs from the one before it by less than tol.  tol=None never reads: exactly max_iter iterations.
    -> (iterations, converged, the last handle)"""
    previous = current = None
    for it in range(1, max_iter + 1):
        previous, current = current, step()
        if tol is not None and (it % check_every == 0 or it == max_iter):
            before, now = read(previous, current)
            if abs(now - before) < tol:
                return it, True, current
    return max_iter, False, current


class GaussianMixture:
    """A mixture of k diagonal Gaussians on device rows [n, dim]; one EM iteration = sv_gmm_estep, sv_gmm_accum, sv_gmm_finish.

    init: "kmeans" (KMeans: k-means++ seeding and a few Lloyd steps, then the M-step of its one-hot responsibilities) or "random" (k
    distinct rows chosen by the seed as means, the per-dimension variance of the rows, equal weights); set_parameters() sets the model
    directly.  reg_covar is added to every variance, as in scikit-learn.  A component that no row is responsible for keeps its mean and
    variance and gets weight 0.  step(), score_samples(), predict(), predict_proba() and sample() issue no host synchronisation and can
    be captured under torch.cuda.graph (after one call outside the capture, which allocates the workspace) and replayed on new rows of
    the same shape."""

    def __init__(self, k, dim, reg_covar=1e-6, init="kmeans", seed=0):
        self.k, self.dim, self.seed, self.reg_covar = int(k), int(dim), int(seed), float(reg_covar)
        if self.k < 1:
            raise ValueError("GaussianMixture: k must be >= 1")
        if not 1 <= self.dim <= MAX_DIM or self.k * (2 * self.dim + 1) >= (1 << 31) - 1:
            raise ValueError("GaussianMixture: dim must be in [1, 2^20] and k (2 dim + 1) below 2^31 (sv_gmm_accum's grid and states)")
        if not (self.reg_covar >= 0.0 and math.isfinite(self.reg_covar)):
            raise ValueError("GaussianMixture: reg_covar must be finite and >= 0")
        if init not in ("kmeans", "random"):
            raise ValueError("GaussianMixture: init must be 'kmeans' or 'random'")
        self.init = init
        self.logw = self.mean = self.var = None        # the model: fp32 [k], [k, dim], [k, dim]
        self._table = None                             # (ivar, cst, cdf), derived by sv_gmm_prepare / sv_gmm_finish
        self._fresh = False                            # the table belongs to the model
        self._work = {}                                # the workspace of step(), by the number of rows
        self.stats = None
        self.converged_, self.n_iter_, self.lower_bound_ = False, 0, None

    # ---- the model ----
    @property
    def weights(self):
        return self.logw.exp()

    def set_parameters(self, weights, means, variances):
        """weights [k] (>= 0, not all 0; stored as their logarithms: a zero is a component that takes part in nothing), means and
        variances [k, dim] (> 0), device tensors"""
        shapes = ((weights, (self.k,)), (means, (self.k, self.dim)), (variances, (self.k, self.dim)))
        for t, shape in shapes:
            if not torch.is_tensor(t) or tuple(t.shape) != shape:
                raise ValueError("GaussianMixture.set_parameters: weights [%d], means and variances [%d, %d]" % (self.k, self.k, self.dim))
        on_device("GaussianMixture.set_parameters", weights, means, variances)
        self.logw = weights.detach().double().log().float().contiguous()
        self.mean = means.detach().float().contiguous().clone()
        self.var = variances.detach().float().contiguous().clone()
        self._fresh = False
        return self

    def _ready(self, what):
        """the model and its table on the device"""
        if self.mean is None:
            raise ValueError("%s: no parameters yet: call fit(), set_parameters() or load_state_dict() first" % what)
        if not self.mean.is_cuda:
            raise L.ShotVaeHipError("%s: the mixture is not on an MI355X (no CPU fallback): load_state_dict(..., device=...)" % what)
        if self._table is None or self._table[0].device != self.mean.device:
            dev = self.mean.device
            self._table = (torch.empty(self.k, self.dim, dtype=torch.float32, device=dev),
                           torch.empty(self.k, dtype=torch.float32, device=dev), torch.empty(self.k, dtype=torch.float32, device=dev))
            self._fresh = False
        if not self._fresh:
            ivar, cst, cdf = self._table
            L.call("sv_gmm_prepare", _p(self.logw), _p(self.mean), _p(self.var), self.k, self.dim, _p(ivar), _p(cst), _p(cdf), _st())
            self._fresh = True
        return self._table

    def _workspace(self, n, dev):
        w = self._work.get(n)
        if w is None or w[0].device != dev:
            P = _partials(self.k, self.dim, n)
            w = (torch.empty(n, dtype=torch.float32, device=dev),
                 torch.empty(P, self.k * (2 * self.dim + 1) + 1, dtype=torch.float64, device=dev),
                 torch.empty(P, 2, dtype=torch.int64, device=dev), P)
            self._work = {n: w}                        # one shape at a time
            if self.stats is None or self.stats.device != dev:
                self.stats = torch.empty(4, dtype=torch.float32, device=dev)
        return w

    def _estep(self, what, x, assign=False, resp=False):
        x = _matrix(what, x, self.dim)
        ivar, cst, _ = self._ready(what)
        n = x.shape[0]
        lse = torch.empty(n, dtype=torch.float32, device=x.device)
        a = torch.empty(n, dtype=torch.int64, device=x.device) if assign else None
        r = torch.empty(n, self.k, dtype=torch.float32, device=x.device) if resp else None
        L.call("sv_gmm_estep", _p(x), n, _p(ivar), _p(self.mean), _p(cst), self.k, self.dim, _p(lse), _p(a), _p(r), _st())
        return lse, a, r

    # ---- EM ----
    def step(self, x):
        """one EM iteration from the current parameters, in place -> stats fp32 [4] on the device (rewritten by the next step): the mean
        log-likelihood of the finite rows under the parameters the step STARTED from (scikit-learn's lower bound), the number of finite
        rows, the number of skipped rows, the smallest variance written"""
        x = _matrix("GaussianMixture.step", x, self.dim)
        ivar, cst, cdf = self._ready("GaussianMixture.step")
        n = x.shape[0]
        lse, sums, counts, P = self._workspace(n, x.device)
        L.call("sv_gmm_estep", _p(x), n, _p(ivar), _p(self.mean), _p(cst), self.k, self.dim, _p(lse), None, None, _st())
        L.call("sv_gmm_accum", _p(x), _p(lse), n, _p(ivar), _p(self.mean), _p(cst), self.k, self.dim, _p(sums), _p(counts), P, 1, _st())
        L.call("sv_gmm_finish", _p(sums), _p(counts), P, self.k, self.dim, self.reg_covar, _p(self.logw), _p(self.mean), _p(self.var),
               _p(ivar), _p(cst), _p(cdf), _p(self.stats), _st())
        return self.stats

    def reset(self, x, generator=None):
        """(re)places the parameters at their initial position: a seeding of the rows x"""
        x = _matrix("GaussianMixture.reset", x, self.dim, k=self.k)
        gen = generator if generator is not None else torch.Generator().manual_seed(self.seed)
        n, dev = x.shape[0], x.device
        spread = x.double().var(dim=0, unbiased=False)
        if self.init == "random":
            mean = x.index_select(0, torch.randperm(n, generator=gen)[:self.k].to(dev)).double()
            var = (spread + self.reg_covar).expand(self.k, self.dim)
            weight = torch.full((self.k,), 1.0 / self.k, dtype=torch.float64, device=dev)
        else:
            # the M-step of one-hot responsibilities: per-cluster sums of x and x^2 in a fixed order (sv_kmeans_accum), divided in double
            km = KMeans(self.k, self.dim, init="k-means++", seed=self.seed)
            km.reset(x, gen)
            for _ in range(KMEANS_STEPS):
                km.step(x)
            assign = km.predict(x)
            P = _kmeans_partials(self.k, self.dim, n)
            sums = torch.empty(2, P, self.k, self.dim, dtype=torch.float64, device=dev)
            counts = torch.empty(P, self.k, dtype=torch.int64, device=dev)
            for i, rows in enumerate((x, (x * x).contiguous())):
                L.call("sv_kmeans_accum", _p(rows), _p(assign), None, n, self.dim, self.k, _p(sums[i]), _p(counts), None, P, 1, _st())
            size = counts.sum(dim=0).double()
            nk = (size + 10.0 * torch.finfo(torch.float64).eps)[:, None]
            s1, s2 = sums.sum(dim=1)
            empty = (size == 0)[:, None]
            mean = torch.where(empty, km.centroids.double(), s1 / nk)
            var = torch.where(empty, spread.expand(self.k, self.dim), s2 / nk - (s1 / nk) ** 2).clamp_min(0.0) + self.reg_covar
            weight = nk[:, 0] / nk.sum()
        self.set_parameters(weight, mean, var)
        self.n_iter_, self.converged_ = 0, False
        return self

    def fit(self, x, max_iter=100, tol=1e-3, check_every=1, n_init=1):
        """EM iterations from a fresh start until the lower bound (the mean log-likelihood, stats[0]) of an iteration differs from that of
        the iteration before by less than tol -- scikit-learn's rule -- or max_iter is reached.  The bound is read on the host once per
        `check_every` iterations; tol=None never reads: exactly max_iter iterations.  n_init > 1 repeats the run with further draws of the
        same generator and keeps the run with the highest bound (chosen on the device: no host read per run).  Afterwards lower_bound_ (a
        fp32 scalar tensor on the device: the bound of the kept run's last iteration) and, of the LAST run, converged_ and n_iter_."""
        max_iter, check_every, n_init = int(max_iter), int(check_every), int(n_init)
        if max_iter < 1 or check_every < 1 or n_init < 1:
            raise ValueError("GaussianMixture.fit: max_iter, check_every and n_init must be >= 1")
        if tol is not None and not float(tol) >= 0.0:
            raise ValueError("GaussianMixture.fit: tol must be >= 0 or None")
        x = _matrix("GaussianMixture.fit", x, self.dim, k=self.k)
        gen = torch.Generator().manual_seed(self.seed)
        minus_inf = torch.full((1,), float("-inf"), dtype=torch.float32, device=x.device)

        def read(previous, current):
            before, now = torch.cat([minus_inf if previous is None else previous, current]).cpu().tolist()
            return before, now

        best = None
        for _ in range(n_init):
            self._table = None                         # (a run's table is kept with its parameters: the next run gets its own)
            self.reset(x, gen)
            self._ready("GaussianMixture.fit")
            self.n_iter_, self.converged_, bound = _em_loop(lambda: self.step(x)[:1].clone(), read, max_iter,
                                                            None if tol is None else float(tol), check_every)
            run = (self.logw, self.mean, self.var) + self._table + (bound,)
            if best is None:
                best = run
            else:
                better = run[-1] > best[-1]
                best = tuple(torch.where(better, a, b) for a, b in zip(run, best))
        self.logw, self.mean, self.var = best[:3]
        self._table, self._fresh = tuple(best[3:6]), True
        self.lower_bound_ = best[6].reshape(())
        return self

    # ---- the density ----
    def score_samples(self, x):
        """-> log p(x_i) under the mixture, fp32 [n] on the device (NaN for a row that is not finite)"""
        return self._estep("GaussianMixture.score_samples", x)[0]

    def score(self, x):
        """-> the SUM of score_samples over the rows, a float64 scalar tensor; it stays on the device"""
        return self.score_samples(x).double().sum()

    def predict(self, x):
        """-> the component of largest weighted density of every row, int64 [n] (the smaller index on a tie; -1 for a row that is not finite)"""
        return self._estep("GaussianMixture.predict", x, assign=True)[1]

    def predict_proba(self, x):
        """-> the responsibilities, fp32 [n, k]: the one call that stores the [rows, components] matrix"""
        return self._estep("GaussianMixture.predict_proba", x, resp=True)[2]

    def bic(self, x):
        """-> -2 log L + (k - 1 + 2 k dim) log n, a float64 scalar tensor on the device (scikit-learn's bic)"""
        return -2.0 * self.score(x) + n_parameters(self.k, self.dim) * math.log(x.shape[0])

    def aic(self, x):
        """-> -2 log L + 2 (k - 1 + 2 k dim), a float64 scalar tensor on the device"""
        return -2.0 * self.score(x) + 2.0 * n_parameters(self.k, self.dim)

    def sample(self, n, key, row0=0, return_component=False):
        """-> z fp32 [n, dim]: row b is drawn from component c(b) -- the first whose cumulative weight exceeds the row's uniform -- as
        mean_c + sqrt(var_c) n(row0 + b, .), sv_latent_draw's counter-based stream under a tag of its own.  A row depends only on
        (key, row0 + b): a batch drawn in one call equals the same rows drawn in several.  key: an int, or a 1-element int64 device tensor
        (read on the device).  return_component: -> (z, c int64 [n])"""
        n, row0 = int(n), int(row0)
        if n < 1 or row0 < 0:
            raise ValueError("GaussianMixture.sample: n must be >= 1 and row0 >= 0")
        _, _, cdf = self._ready("GaussianMixture.sample")
        dev = self.mean.device
        key = _key_tensor("GaussianMixture.sample", key, dev)
        z = torch.empty(n, self.dim, dtype=torch.float32, device=dev)
        comp = torch.empty(n, dtype=torch.int64, device=dev) if return_component else None
        L.call("sv_gmm_sample", _p(self.mean), _p(self.var), _p(cdf), self.k, self.dim, _p(key), row0, n, _p(z), _p(comp), _st())
        return (z, comp) if return_component else z

    # ---- checkpoints ----
    def state_dict(self):
        if self.mean is None:
            raise ValueError("GaussianMixture.state_dict: no parameters yet")
        return dict(k=self.k, dim=self.dim, reg_covar=self.reg_covar, logw=self.logw.clone(), mean=self.mean.clone(), var=self.var.clone(),
                    converged=bool(self.converged_), n_iter=int(self.n_iter_))

    def load_state_dict(self, state, device=None):
        """takes a state_dict() (tensors on any device; `device`: where to put them).  Nothing runs here: the table is derived at the
        first use, which refuses a mixture that is still on the host."""
        if int(state["k"]) != self.k or int(state["dim"]) != self.dim:
            raise ValueError("GaussianMixture.load_state_dict: the state is %d x %d, the mixture %d x %d"
                             % (int(state["k"]), int(state["dim"]), self.k, self.dim))
        for name, shape in (("logw", (self.k,)), ("mean", (self.k, self.dim)), ("var", (self.k, self.dim))):
            if not torch.is_tensor(state[name]) or tuple(state[name].shape) != shape:
                raise ValueError("GaussianMixture.load_state_dict: %s must be a tensor %s" % (name, list(shape)))
        put = (lambda t: t.detach().float().contiguous().clone()) if device is None else (lambda t: t.detach().float().to(device).contiguous().clone())
        self.logw, self.mean, self.var = put(state["logw"]), put(state["mean"]), put(state["var"])
        self.reg_covar = float(state.get("reg_covar", self.reg_covar))
        self.converged_, self.n_iter_ = bool(state.get("converged", False)), int(state.get("n_iter", 0))
        self._fresh = False
        return self


def evaluate_mixture(model, fit_batches, test_batches=None, k=10, space="mu", **fit_args):
    """How much better than the prior does a mixture of k diagonal Gaussians describe the codes of `model` (a VariationalAutoEncoder or a
    SmoothVAE, in eval mode: NotImplementedError otherwise, as for score)?  fit_batches / test_batches: (image, label) or (image,) tuples,
    or image tensors, on the device.  A GaussianMixture(k, **fit_args: reg_covar, init, seed, and fit's max_iter, tol, check_every,
    n_init) is fitted to the posterior means (space "mu", the only space) of ALL rows of fit_batches, gathered first: the result does
    not depend on the batching.  -> a dict:

        ll_fit, ll_test              the mean log-likelihood of the fit / test rows under the mixture (ll_test None without test_batches)
        prior_ll_fit, prior_ll_test  the same under the prior N(0, I): -(d log 2 pi + mean |mu|^2) / 2, float64 from device sums
        bic, aic                     of the fit set;   n_fit, n_test;   n_parameters
        partition_fit, partition_test  partition_metrics of predict() against the labels (classes of the discrete code x components),
                                     None where the batches carry no labels
        mixture                      the fitted GaussianMixture

    One host read at the end beyond those of fit."""
    latent_family("evaluate_mixture", model)
    if space != "mu":
        raise ValueError("evaluate_mixture: space must be 'mu'")
    eval_only("evaluate_mixture", model)
    run_args = take_args(fit_args, ("max_iter", "tol", "check_every", "n_init"))
    classes = num_classes(model)
    k = int(k)

    def codes(batches):
        mu, _, label = gather_codes("evaluate_mixture", model, batches, need_label=False)
        return mu, label

    sets = [codes(fit_batches)] + ([codes(test_batches)] if test_batches is not None else [])
    dim = sets[0][0].shape[1]
    gm = GaussianMixture(k, dim, **fit_args).fit(sets[0][0], **run_args)
    packed, tables = [], []
    for mu, label in sets:
        packed += [gm.score(mu).reshape(1), (mu.double() ** 2).sum().reshape(1)]
        if label is not None:
            tables.append(contingency(label, gm.predict(mu), classes, k).reshape(-1).double())
    host = torch.cat(packed + tables).cpu().numpy()

    res, at = dict(mixture=gm, n_parameters=n_parameters(k, dim), ll_test=None, prior_ll_test=None, n_test=0, partition_fit=None,
                   partition_test=None), 2 * len(sets)
    for i, (name, (mu, label)) in enumerate(zip(("fit", "test"), sets)):
        n = mu.shape[0]
        res["n_" + name] = n
        res["ll_" + name] = float(host[2 * i]) / n
        res["prior_ll_" + name] = -0.5 * (dim * math.log(2.0 * math.pi) + float(host[2 * i + 1]) / n)
        if label is not None:
            table = host[at:at + classes * k].round().astype("int64").reshape(classes, k)
            at += classes * k
            res["partition_" + name] = partition_metrics(table) if table.sum() > 0 else None
    n = res["n_fit"]
    res["bic"] = -2.0 * float(host[0]) + res["n_parameters"] * math.log(n)
    res["aic"] = -2.0 * float(host[0]) + 2.0 * res["n_parameters"]
    return res


def generate_from_mixture(model, mixture, labels, key, row0=0, **decode_args):
    """Class-conditional images of codes drawn from a fitted mixture where generate() draws from the prior: z = mixture.sample(len(labels),
    key, row0), then model.decode(z, labels, **decode_args) (a VariationalAutoEncoder; sigmoid=True unless said otherwise: the images
    generate() gives) or model.decode([z | one-hot(labels)]) (a SmoothVAE; a label outside the code sets no class).  A row depends only
    on (key, row0 + its row), as in generate()."""
    family = latent_family("generate_from_mixture", model)
    if not isinstance(mixture, GaussianMixture):
        raise TypeError("generate_from_mixture: a GaussianMixture, not %s" % type(mixture).__name__)
    if not torch.is_tensor(labels) or labels.dtype != torch.int64 or labels.numel() < 1:
        raise ValueError("generate_from_mixture: labels must be a non-empty int64 vector on the device")
    on_device("generate_from_mixture", labels)
    labels = labels.reshape(-1).contiguous()
    z = mixture.sample(labels.numel(), key, row0=row0)
    if family == "shot":
        if mixture.dim != model._plan.ldc:
            raise ValueError("generate_from_mixture: the mixture has %d dimensions, the model's code %d" % (mixture.dim, model._plan.ldc))
        decode_args.setdefault("sigmoid", True)
        return model.decode(z, labels, **decode_args)
    if mixture.dim != model.latent_cont_dim:
        raise ValueError("generate_from_mixture: the mixture has %d dimensions, the model's code %d" % (mixture.dim, model.latent_cont_dim))
    if decode_args:
        raise ValueError("generate_from_mixture: a SmoothVAE's decode takes no arguments")
    with torch.no_grad():
        Dd = model.latent_disc_dim
        hot = (labels[:, None] == torch.arange(Dd, device=labels.device)[None, :]).float()
        return model.decode(torch.cat([z, hot], dim=1))
