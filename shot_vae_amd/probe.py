"""The linear evaluation protocol: a multinomial logistic regression on the frozen codes, fitted by fused Nesterov iterations on the HIP
path (csrc/probe.hip).

    lp = LinearProbe(10, 128, C=1.0).fit(mu, y)                        # y int64 [n]; a label outside [0, 10) (-1) is an unlabelled row
    lp.predict(mu), lp.predict_proba(mu)                               # the first maximum, the probabilities
    lp.score(mu, y), lp.log_loss(mu, y)                                # accuracy and mean negative log-likelihood, on the device
    lp.decision_function(mu)                                           # [n, 10] logits for calibration.row_stats / TemperatureScaler
    evaluate_probe(model, fit_loader, test_loader, labels_per_class=[10, 100, None])      # the accuracy over the label budget

The objective is scikit-learn's LogisticRegression(C=C) over C n: 1/n sum_i (lse_i - v(i, y_i)) + lambda / 2 |w|^2 with lambda =
1 / (C n) and an unpenalised intercept.  Rows must be finite: a NaN or infinite row has loss NaN, is predicted as -1 and enters no
gradient.  The [rows, classes] matrix exists only where predict_proba or decision_function ask for it, there is no atomic of any kind --
the same call sequence gives the same bits --, nothing here synchronises with the host except where stated, and there is no CPU
fallback."""
import math

import torch

from . import _lib as L
from .aggregate import partials
from ._latent import (_p, _st, eval_only, gather_codes, label_budgets, labels as _labels, latent_family, matrix, num_classes,
                      resident_partials, take_args)

MAX_DIM = 1 << 20             # sv_probe_accum: a block owns 32 dimensions, the grid's second dimension holds 65535 blocks
SLICE = 32
BLOCKS_PER_CU = 2             # sv_probe_accum's blocks resident per compute unit (its launch bound)


def _partials(k, dim, n):
    """P of sv_probe_accum for n rows: mixture._partials' rule over this kernel's grid of ceil(k / tile) x ceil(dim / 32) blocks per state
    (tile = 16 classes for k <= 16, else 64), lowered until the grid is resident at once.  A function of the shapes alone."""
    blocks = (1 if k <= 16 else -(-k // 64)) * -(-dim // SLICE)
    return resident_partials(partials(blocks, n), blocks, BLOCKS_PER_CU)


def _matrix(what, x, dim=None):
    return matrix(what, x, dim, "the probe")


def _probe_loop(step, read, max_iter, tol, check_every):
    """The iterations of one fit and scikit-learn's lbfgs stopping rule.  step() runs one iteration and returns a handle of its max |g|;
    read(handle) brings it to the host as a float.  It is read once per `check_every` iterations and at the last one; the run has
    converged when it is below tol.  tol=None never reads: exactly max_iter iterations.  -> (iterations, converged)"""
    for it in range(1, max_iter + 1):
        current = step()
        if tol is not None and (it % check_every == 0 or it == max_iter):
            if read(current) < tol:
                return it, True
    return max_iter, False


def step_constants(eigmax, lam):
    """-> (L, beta) of the constant-momentum method: L = eigmax / 2 + lambda is Boehning's bound on the Hessian of the softmax loss
    (eigmax: the largest eigenvalue of the Gram matrix of [x, 1] over n), and beta = (1 - sqrt(lambda / L)) / (1 + sqrt(lambda / L))"""
    lip = 0.5 * float(eigmax) + float(lam)
    q = math.sqrt(float(lam) / lip)
    return lip, (1.0 - q) / (1.0 + q)


def select_labels(y, per_class, num_classes, seed=0):
    """The label budget: under ONE permutation of the rows drawn from `seed`, the first `per_class` rows of every class keep their label
    and every other row gets -1 (a class with fewer rows keeps all of them).  The budgets are nested: a row labelled under m is labelled
    under every m' >= m.  Works where y lives (no host read); rows whose label is outside [0, num_classes) stay unlabelled."""
    if not torch.is_tensor(y) or y.dim() != 1 or y.dtype.is_floating_point or y.dtype == torch.bool:
        raise ValueError("select_labels: y must be an integer vector")
    per_class, num_classes = int(per_class), int(num_classes)
    if per_class < 1 or num_classes < 1:
        raise ValueError("select_labels: per_class and num_classes must be >= 1")
    y = y.long()
    n = y.shape[0]
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(int(seed))).to(y.device)
    yp = y[perm]
    valid = (yp >= 0) & (yp < num_classes)
    key = torch.where(valid, yp, torch.full_like(yp, num_classes))
    order = torch.sort(key, stable=True).indices                 # the classes in blocks, each in the permutation's order
    sorted_key = key[order]
    size = torch.zeros(num_classes + 1, dtype=torch.int64, device=y.device).scatter_add_(0, sorted_key, torch.ones_like(sorted_key))
    first = torch.cumsum(size, 0) - size
    rank = torch.arange(n, device=y.device) - first[sorted_key]
    keep = (rank < per_class) & (sorted_key < num_classes)
    out = torch.full_like(y, -1)
    rows = perm[order]
    out[rows] = torch.where(keep, sorted_key, torch.full_like(sorted_key, -1))
    return out


class LinearProbe:
    """Multinomial logistic regression on device rows [n, dim]; one iteration = sv_probe_rows, sv_probe_accum, sv_probe_update: Nesterov's
    method with constant momentum from theta = 0.

    C is scikit-learn's inverse regularisation strength (lambda = 1 / (C n)).  standardize: the rows are centred and scaled per dimension
    by the statistics of the labelled fit rows before anything else (the default: on correlated rows of mean 3 the solver was still at
    max |g| = 6e-3 after 400 iterations where the standardised rows had reached 3e-7 after 200); the penalty then acts on the weights of
    the standardised rows, and coef_ / intercept_ translate them back.  step(), predict(), predict_proba(), decision_function(), score()
    and log_loss() issue no host synchronisation; step() can be captured under torch.cuda.graph (after one call outside the capture,
    which allocates the workspace) and replayed on new rows of the same shape."""

    def __init__(self, num_classes, dim, C=1.0, standardize=True):
        self.k, self.dim, self.C, self.standardize = int(num_classes), int(dim), float(C), bool(standardize)
        if self.k < 2:
            raise ValueError("LinearProbe: num_classes must be >= 2")
        if not 1 <= self.dim <= MAX_DIM or self.k * (self.dim + 1) >= (1 << 31) - 1:
            raise ValueError("LinearProbe: dim must be in [1, 2^20] and num_classes (dim + 1) below 2^31 (sv_probe_accum's grid and states)")
        if not (self.C > 0.0 and math.isfinite(self.C)):
            raise ValueError("LinearProbe: C must be finite and > 0")
        self.w = self.b = None                         # the model the scans read: fp32 [k, dim], [k] -- the look-ahead point, rounded once
        self.theta = self.look = None                  # the iterates, float64 [k, dim + 1]: column 0 is the intercept
        self.mean = self.scale = None                  # the standardisation, float64 [dim] (0 and 1 without)
        self.lam = self.lipschitz = self.beta = None
        self._work = {}                                # the workspace of step(), by the number of rows
        self.stats = None
        self.converged_, self.n_iter_ = False, 0

    # ---- the model ----
    def _ready(self, what):
        if self.w is None:
            raise ValueError("%s: no parameters yet: call fit() or load_state_dict() first" % what)
        if not self.w.is_cuda:
            raise L.ShotVaeHipError("%s: the probe is not on an MI355X (no CPU fallback): load_state_dict(..., device=...)" % what)

    def _rows(self, what, x):
        """the rows as the scans read them: standardised in torch, one rounding to fp32"""
        if self.w is None:
            raise ValueError("%s: no parameters yet: call fit() or load_state_dict() first" % what)
        x = _matrix(what, x, self.dim)
        self._ready(what)
        if not self.standardize:
            return x
        return ((x.double() - self.mean) / self.scale).float().contiguous()

    def start(self, dev, lam, lipschitz, beta, mean=None, scale=None):
        """(re)places the iterates at 0 with the constants of a fit: lambda, L and beta (step_constants), and the standardisation"""
        lam, lipschitz, beta = float(lam), float(lipschitz), float(beta)
        if not (lam > 0.0 and math.isfinite(lam) and lipschitz > 0.0 and math.isfinite(lipschitz) and 0.0 <= beta < 1.0):
            raise ValueError("LinearProbe.start: lambda and L must be finite and > 0, beta in [0, 1)")
        if torch.device(dev).type != "cuda":
            raise L.ShotVaeHipError("LinearProbe.start: the device is not an MI355X (no CPU fallback)")
        self.lam, self.lipschitz, self.beta = lam, lipschitz, beta
        self.w = torch.zeros(self.k, self.dim, dtype=torch.float32, device=dev)
        self.b = torch.zeros(self.k, dtype=torch.float32, device=dev)
        self.theta = torch.zeros(self.k, self.dim + 1, dtype=torch.float64, device=dev)
        self.look = torch.zeros(self.k, self.dim + 1, dtype=torch.float64, device=dev)
        self.mean = torch.zeros(self.dim, dtype=torch.float64, device=dev) if mean is None else mean.double().to(dev)
        self.scale = torch.ones(self.dim, dtype=torch.float64, device=dev) if scale is None else scale.double().to(dev)
        self.n_iter_, self.converged_ = 0, False
        return self

    def _workspace(self, n, dev):
        w = self._work.get(n)
        if w is None or w[0].device != dev:
            P = _partials(self.k, self.dim, n)
            w = (torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev),
                 torch.empty(P, self.k * (self.dim + 1) + 1, dtype=torch.float64, device=dev),
                 torch.empty(P, 2, dtype=torch.int64, device=dev), P)
            self._work = {n: w}                        # one shape at a time
            if self.stats is None or self.stats.device != dev:
                self.stats = torch.empty(4 + 2 * self.k, dtype=torch.float64, device=dev)
        return w

    def _scan(self, what, x, labelled=False, y=None, pred=False, proba=False):
        x = self._rows(what, x)
        n = x.shape[0]
        y = _labels(what, y, n) if labelled else None
        lse = torch.empty(n, dtype=torch.float32, device=x.device)
        loss = torch.empty(n, dtype=torch.float32, device=x.device) if y is not None else None
        a = torch.empty(n, dtype=torch.int64, device=x.device) if pred else None
        r = torch.empty(n, self.k, dtype=torch.float32, device=x.device) if proba else None
        L.call("sv_probe_rows", _p(x), n, _p(self.w), _p(self.b), self.k, self.dim, _p(y), _p(lse), _p(loss), _p(a), _p(r), _st())
        return lse, loss, a, r, y

    # ---- the solver ----
    def step(self, x, y):
        """one iteration on rows AS THE SCANS READ THEM (fit standardises first), in place -> stats float64 [4 + 2 k] on the device
        (rewritten by the next step): the objective at the look-ahead point the step STARTED from, max |g| there, the rows used, the rows
        skipped, then the class partials"""
        x = _matrix("LinearProbe.step", x, self.dim)
        y = _labels("LinearProbe.step", y, x.shape[0])
        self._ready("LinearProbe.step")
        if self.lam is None:
            raise ValueError("LinearProbe.step: no step constants yet: call start() or fit() first")
        n = x.shape[0]
        lse, loss, sums, counts, P = self._workspace(n, x.device)
        L.call("sv_probe_rows", _p(x), n, _p(self.w), _p(self.b), self.k, self.dim, _p(y), _p(lse), _p(loss), None, None, _st())
        L.call("sv_probe_accum", _p(x), _p(y), _p(lse), _p(loss), n, _p(self.w), _p(self.b), self.k, self.dim, _p(sums), _p(counts), P, 1,
               None, _st())
        L.call("sv_probe_update", _p(sums), _p(counts), P, self.k, self.dim, self.lam, 1.0 / self.lipschitz, self.beta, _p(self.theta),
               _p(self.look), _p(self.w), _p(self.b), _p(self.stats), _st())
        return self.stats

    def prepare(self, x, y):
        """What fit does before its first step, in torch, in this order: per-dimension mean and standard deviation over the used rows
        (label in [0, k), every entry finite); a standardised fp32 copy of the rows if standardize is set; the largest eigenvalue of the
        (dim + 1) x (dim + 1) Gram matrix of [x, 1] over the used rows, divided by n, in float64; L = eigmax / 2 + lambda; beta.  ONE host
        read covers all of it: the Gram matrix and n come to the host together and the eigenvalue is taken there.  -> the rows the steps
        read"""
        x = _matrix("LinearProbe.fit", x, self.dim)
        y = _labels("LinearProbe.fit", y, x.shape[0])
        used = ((y >= 0) & (y < self.k) & torch.isfinite(x).all(dim=1)).double()[:, None]
        xd = torch.where(used > 0, x.double(), torch.zeros((), dtype=torch.float64, device=x.device))
        n = used.sum()
        mean = xd.sum(dim=0) / n
        if self.standardize:
            var = (((xd - mean) * used) ** 2).sum(dim=0) / n
            scale = torch.where(var > 0, var.sqrt(), torch.ones_like(var))
            rows = ((x.double() - mean) / scale).float().contiguous()
        else:
            mean, scale, rows = torch.zeros_like(mean), torch.ones_like(mean), x
        aug = torch.cat([torch.where(used > 0, rows.double(), torch.zeros((), dtype=torch.float64, device=x.device)), used], dim=1)
        gram = aug.T @ aug
        host = torch.cat([gram.reshape(-1), n.reshape(1)]).cpu()                    # the one host read
        count = int(host[-1].item())
        if count < 1:
            raise ValueError("LinearProbe.fit: no labelled finite row")
        eigmax = float(torch.linalg.eigvalsh(host[:-1].reshape(self.dim + 1, self.dim + 1) / count)[-1])
        lam = 1.0 / (self.C * count)
        lipschitz, beta = step_constants(eigmax, lam)
        self.start(x.device, lam, lipschitz, beta, mean, scale)
        return rows, y

    def fit(self, x, y, max_iter=2000, tol=1e-4, check_every=10):
        """Iterations from theta = 0 until max |g| -- the largest entry of the gradient of the objective at the look-ahead point --
        is below tol (scikit-learn's lbfgs criterion) or max_iter is reached.  Before the first step prepare() reads the Gram matrix once
        on the host; max |g| is then read once per `check_every` iterations, and tol=None never reads: exactly max_iter iterations.
        Afterwards converged_ and n_iter_."""
        max_iter, check_every = int(max_iter), int(check_every)
        if max_iter < 1 or check_every < 1:
            raise ValueError("LinearProbe.fit: max_iter and check_every must be >= 1")
        if tol is not None and not float(tol) >= 0.0:
            raise ValueError("LinearProbe.fit: tol must be >= 0 or None")
        rows, y = self.prepare(x, y)
        self.n_iter_, self.converged_ = _probe_loop(lambda: self.step(rows, y)[1:2].clone(), lambda h: float(h.cpu()[0]), max_iter,
                                                    None if tol is None else float(tol), check_every)
        return self

    # ---- the classifier ----
    def predict(self, x):
        """-> the class of largest score of every row, int64 [n] (the smaller index on a tie; -1 for a row that is not finite)"""
        return self._scan("LinearProbe.predict", x, pred=True)[2]

    def predict_proba(self, x):
        """-> the class probabilities, fp32 [n, k]: a call that stores the [rows, classes] matrix"""
        return self._scan("LinearProbe.predict_proba", x, proba=True)[3]

    def decision_function(self, x):
        """-> the logits, fp32 [n, k], for calibration.row_stats / Reliability / TemperatureScaler: the one call that materialises them,
        on request -- the products and the sum in float64 in torch, rounded once (within an fp32 rounding of the scans' v, which round
        their 16-blocks)"""
        x = self._rows("LinearProbe.decision_function", x)
        return torch.addmm(self.b.double(), x.double(), self.w.double().T).float()

    def score(self, x, y):
        """-> the accuracy over the labelled rows (label in [0, k)), a float64 scalar tensor; it stays on the device"""
        _, _, pred, _, y = self._scan("LinearProbe.score", x, True, y, pred=True)
        labelled = (y >= 0) & (y < self.k)
        return ((pred == y) & labelled).double().sum() / labelled.double().sum()

    def log_loss(self, x, y):
        """-> the mean of lse_i - v(i, y_i) over the labelled rows, a float64 scalar tensor on the device (NaN if one of them is not
        finite)"""
        _, loss, _, _, y = self._scan("LinearProbe.log_loss", x, True, y)
        labelled = (y >= 0) & (y < self.k)
        return torch.where(labelled, loss.double(), torch.zeros((), dtype=torch.float64, device=loss.device)).sum() / labelled.double().sum()

    @property
    def coef_(self):
        """the weights in the coordinates of the RAW rows, float64 [k, dim]: v = intercept_ + coef_ x"""
        self._ready("LinearProbe.coef_")
        return self.w.double() / self.scale

    @property
    def intercept_(self):
        self._ready("LinearProbe.intercept_")
        return self.b.double() - (self.w.double() * (self.mean / self.scale)).sum(dim=1)

    # ---- checkpoints ----
    def state_dict(self):
        if self.w is None:
            raise ValueError("LinearProbe.state_dict: no parameters yet")
        return dict(k=self.k, dim=self.dim, C=self.C, standardize=self.standardize, w=self.w.clone(), b=self.b.clone(),
                    mean=self.mean.clone(), scale=self.scale.clone(), converged=bool(self.converged_), n_iter=int(self.n_iter_))

    def load_state_dict(self, state, device=None):
        """takes a state_dict() (tensors on any device; `device`: where to put them).  Nothing runs here: the first use refuses a probe
        that is still on the host.  The iterates restart at the loaded point."""
        if int(state["k"]) != self.k or int(state["dim"]) != self.dim:
            raise ValueError("LinearProbe.load_state_dict: the state is %d x %d, the probe %d x %d"
                             % (int(state["k"]), int(state["dim"]), self.k, self.dim))
        for name, shape in (("w", (self.k, self.dim)), ("b", (self.k,)), ("mean", (self.dim,)), ("scale", (self.dim,))):
            if not torch.is_tensor(state[name]) or tuple(state[name].shape) != shape:
                raise ValueError("LinearProbe.load_state_dict: %s must be a tensor %s" % (name, list(shape)))
        put = (lambda t: t.detach().contiguous().clone()) if device is None else (lambda t: t.detach().to(device).contiguous().clone())
        self.w, self.b = put(state["w"].float()), put(state["b"].float())
        self.mean, self.scale = put(state["mean"].double()), put(state["scale"].double())
        self.theta = torch.cat([self.b.double()[:, None], self.w.double()], dim=1).contiguous()
        self.look = self.theta.clone()
        self.C, self.standardize = float(state.get("C", self.C)), bool(state.get("standardize", self.standardize))
        self.converged_, self.n_iter_ = bool(state.get("converged", False)), int(state.get("n_iter", 0))
        return self


def evaluate_probe(model, fit_batches, test_batches, space="mu", labels_per_class=None, seed=0, **probe_args):
    """The linear evaluation protocol on the codes of `model` (a VariationalAutoEncoder or a SmoothVAE, in eval mode: NotImplementedError
    otherwise, as for score): a LinearProbe(classes, d, **probe_args: C, standardize, and fit's max_iter, tol, check_every) is fitted to
    the rows of fit_batches and scored on those of test_batches -- (image, label) tuples on the device.  space: "mu", the posterior
    means, or "features", model.features() where the model has it.  All rows are gathered first: the result does not depend on the
    batching.  labels_per_class: None (all labels), a budget m, or a list of budgets (None among them: all): under ONE permutation
    drawn from `seed` the first m rows of each class keep their label, the rest get -1 (select_labels); the same gathered rows serve
    every budget.  -> a dict budget -> dict:

        n_labelled                   the rows that kept a label
        accuracy_fit                 over the labelled fit rows;   accuracy_test, nll_test   over the test rows
        n_iter, converged            of the fit;   probe   the fitted LinearProbe

    Beyond fit's host reads, one host read per budget."""
    latent_family("evaluate_probe", model)
    if space not in ("mu", "features"):
        raise ValueError("evaluate_probe: space must be 'mu' or 'features'")
    if space == "features" and not hasattr(model, "features"):
        raise ValueError("evaluate_probe: %s has no features(): use space='mu'" % type(model).__name__)
    eval_only("evaluate_probe", model)
    budgets = label_budgets("evaluate_probe", labels_per_class)
    run_args = take_args(probe_args, ("max_iter", "tol", "check_every"))
    classes = num_classes(model)

    x_fit, _, y_fit = gather_codes("evaluate_probe", model, fit_batches, space)
    x_test, _, y_test = gather_codes("evaluate_probe", model, test_batches, space)
    res = {}
    for m in budgets:
        y = y_fit if m is None else select_labels(y_fit, int(m), classes, seed)
        lp = LinearProbe(classes, x_fit.shape[1], **probe_args).fit(x_fit, y, **run_args)
        labelled = ((y >= 0) & (y < classes)).double().sum()
        host = torch.stack([labelled, lp.score(x_fit, y), lp.score(x_test, y_test), lp.log_loss(x_test, y_test)]).cpu().tolist()
        res[m] = dict(n_labelled=int(round(host[0])), accuracy_fit=host[1], accuracy_test=host[2], nll_test=host[3], n_iter=lp.n_iter_,
                      converged=lp.converged_, probe=lp)
    return res
