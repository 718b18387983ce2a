"""Graph-based semi-supervised learning on the codes: label spreading (Zhou et al. 2004) and label propagation (Zhu & Ghahramani 2002)
along the k-NN graph of the posteriors, on the HIP path (csrc/labelprop.hip).

    lp = LabelPropagator(10, variant="spreading", alpha=0.2, k=7, metric="kl").fit(mu, ls, y)     # y int64 [N]; -1: an unlabelled row
    lp.label_distributions_, lp.transduction_, lp.n_iter_, lp.delta_, lp.n_unreached_             # scikit-learn's attributes, on the device
    lp.predict(mu_new, ls_new), lp.predict_proba(mu_new, ls_new)                                  # the mean over the k nearest fitted rows
    evaluate_propagation(model, fit_loader, test_loader, labels_per_class=[10, 100])              # the accuracy over the label budget

The graph is LatentIndex.search's k-lists ("kl" / "w2" / "euclid"; "cosine" holds similarities and is refused), weighted 1
("connectivity") or by embed.conditional_affinities ("affinity"), and symmetrised by embed.symmetrize; its 1 / (2N) scale cancels in
both normalisations.  An iteration is ONE sv_lp_step: a CSR gather with double accumulation in segment order and the variant's clamp.
No atomic anywhere -- the same call sequence gives the same bits --, step() does not synchronise with the host and can be captured, and
there is no CPU fallback."""
import torch

from . import _lib as L
from ._latent import _p, _st, eval_only, gather_codes, label_budgets, labels as _labels, latent_family, num_classes, on_device
from .embed import conditional_affinities, symmetrize
from .neighbors import MAX_K, LatentIndex
from .probe import select_labels

MAX_CLASSES = 1024            # sv_lp_step
VARIANTS = {"spreading": L.LP_SPREADING, "propagation": L.LP_PROPAGATION}
MODES = {"sym": L.LP_SYM, "row": L.LP_ROW}
_GRAPH_METRICS = ("kl", "w2", "wasserstein", "euclid", "euclidean")


def step_scratch(n, k):
    """the number of doubles sv_lp_step needs as scratch for n rows of k classes: two per block of 16 (k <= 16) or 4 rows"""
    return 2 * (-(-int(n) // (16 if int(k) <= 16 else 4)))


def _csr(what, rowptr, col, val):
    """the CSR triple as contiguous device tensors; the shape checks come first (they need no device), then the no-CPU rule"""
    if not all(torch.is_tensor(t) and t.dim() == 1 for t in (rowptr, col, val)) or rowptr.shape[0] < 2 or col.shape != val.shape \
            or rowptr.dtype != torch.int64 or col.dtype != torch.int64:
        raise ValueError("%s: rowptr int64 [N + 1], col int64 [nnz] and val [nnz]" % what)
    on_device(what, rowptr, col, val)
    return rowptr.contiguous(), col.contiguous(), val.detach().float().contiguous()


def knn_graph(mu, ls=None, k=7, metric="kl", weights="connectivity", perplexity=None):
    """The symmetric k-NN graph of the posteriors (mu, ls) [N, dim] as CSR -> (rowptr int64 [N + 1], col int64 [nnz], val fp32 [nnz]):
    every row's k nearest rows under `metric` (LatentIndex.search, the row itself left out; ls = log sigma, None for "euclid"), each
    slot weighted 1 (weights="connectivity") or by its conditional affinity at `perplexity` (weights="affinity"; default
    max(2, k / 3), as TSNE pairs them), then embed.symmetrize: (A + A^T) / (2N) over the union of the edges."""
    if metric not in _GRAPH_METRICS:
        raise ValueError("knn_graph: metric must be 'kl', 'w2' or 'euclid' ('cosine' holds similarities, not distances); got %r" % (metric,))
    if weights not in ("connectivity", "affinity"):
        raise ValueError("knn_graph: weights must be 'connectivity' or 'affinity'; got %r" % (weights,))
    if not torch.is_tensor(mu) or mu.dim() != 2 or mu.shape[0] < 2:
        raise ValueError("knn_graph: mu must be a matrix [N >= 2, dim]")
    k = int(k)
    if not 1 <= k <= min(MAX_K, mu.shape[0] - 1):
        raise ValueError("knn_graph: k must be in [1, min(%d, N - 1 = %d)]; got %d" % (MAX_K, mu.shape[0] - 1, k))
    on_device("knn_graph", mu, ls)
    index = LatentIndex(mu.shape[1], metric)
    index.add(mu, ls)
    dist, idx = index.search(mu, ls, k=k, exclude_self_from=0)
    if weights == "connectivity":
        p = (idx >= 0).float()
    else:
        p = conditional_affinities(dist, idx, max(2.0, k / 3.0) if perplexity is None else float(perplexity))[0]
    return symmetrize(p, idx)


def normalize_graph(rowptr, col, val, mode="sym"):
    """The iteration matrix of a square CSR graph (sv_lp_normalize) -> (sval fp32 [nnz], deg float64 [N]): mode "sym" is Zhou et
    al.'s D^-1/2 W D^-1/2 (scikit-learn's LabelSpreading), "row" is D^-1 W (its LabelPropagation for a symmetric W).  A row of degree 0
    gives zeros, never a NaN; a column outside [0, N) is no edge."""
    if mode not in MODES:
        raise ValueError("normalize_graph: mode must be 'sym' or 'row'; got %r" % (mode,))
    rowptr, col, val = _csr("normalize_graph", rowptr, col, val)
    n, nnz = rowptr.shape[0] - 1, col.shape[0]
    sval = torch.empty(nnz, dtype=torch.float32, device=rowptr.device)
    deg = torch.empty(n, dtype=torch.float64, device=rowptr.device)
    L.call("sv_lp_normalize", _p(rowptr), _p(col) if nnz else None, _p(val) if nnz else None, n, nnz, MODES[mode], _p(deg),
           _p(sval) if nnz else None, _st())
    return sval, deg


def _lp_loop(step, read, max_iter, tol, check_every):
    """The iterations of one fit and scikit-learn's stopping rule: step() runs one iteration and returns a handle of its delta_l1 =
    sum |F_t - F_t-1|; read(handle) brings it to the host as a float.  It is read once per `check_every` iterations, never at
    max_iter (scikit-learn does not look at the last product either); the run has converged when it is below tol.
    -> (iterations, converged, the last delta read or None)"""
    delta = None
    for it in range(1, max_iter + 1):
        current = step()
        if it % check_every == 0 and it < max_iter:
            delta = read(current)
            if delta < tol:
                return it, True, delta
    return max_iter, False, delta


class LabelPropagator:
    """Label spreading / propagation of `num_classes` classes over a symmetric graph.

    variant="spreading": F <- alpha S F + (1 - alpha) Y with S = D^-1/2 W D^-1/2 (scikit-learn's LabelSpreading; alpha in (0, 1));
    variant="propagation": F <- D^-1 W F, every row normalised and the labelled rows reset to their one-hot each iteration (its
    LabelPropagation).  max_iter defaults to scikit-learn's 30 / 1000, tol to its 1e-3, and the graph arguments (k=7, metric="kl",
    weights="connectivity", perplexity) go to knn_graph.

    prepare() builds the graph, its normalisation, two buffers initialised to the one-hot labels and the scratch; step() is one
    sv_lp_step from the current buffer into the other, after which they change roles.  step() issues no host synchronisation and
    can be captured under torch.cuda.graph; A CAPTURED GRAPH MUST HOLD AN EVEN NUMBER OF STEPS, so that every replay starts from the
    buffer the capture started from.  reset() puts the one-hot labels (new ones, if given) back by device copies: one captured graph
    serves any labels.  After fit(): label_distributions_ (fp32 [N, K], rows sum to 1; a row no label reached is 0),
    transduction_ (int64 [N]; -1 on such a row), n_iter_, converged_, delta_ (the last delta_l1 read) and n_unreached_."""

    def __init__(self, num_classes, variant="spreading", alpha=0.2, max_iter=None, tol=1e-3, k=7, metric="kl", weights="connectivity",
                 perplexity=None):
        self.k_classes, self.variant = int(num_classes), variant
        if not 1 <= self.k_classes <= MAX_CLASSES:
            raise ValueError("LabelPropagator: num_classes must be in [1, %d]" % MAX_CLASSES)
        if variant not in VARIANTS:
            raise ValueError("LabelPropagator: variant must be 'spreading' or 'propagation'; got %r" % (variant,))
        self.alpha = float(alpha)
        if variant == "spreading" and not 0.0 < self.alpha < 1.0:
            raise ValueError("LabelPropagator: alpha must be in (0, 1)")
        self.max_iter = (30 if variant == "spreading" else 1000) if max_iter is None else int(max_iter)
        self.tol = float(tol)
        if self.max_iter < 1 or not self.tol >= 0.0:
            raise ValueError("LabelPropagator: max_iter must be >= 1 and tol >= 0")
        if metric not in _GRAPH_METRICS:
            raise ValueError("LabelPropagator: metric must be 'kl', 'w2' or 'euclid' ('cosine' holds similarities, not distances); got %r"
                             % (metric,))
        if weights not in ("connectivity", "affinity"):
            raise ValueError("LabelPropagator: weights must be 'connectivity' or 'affinity'; got %r" % (weights,))
        self.k, self.metric, self.weights, self.perplexity = int(k), metric, weights, perplexity
        if not 1 <= self.k <= MAX_K:
            raise ValueError("LabelPropagator: k must be in [1, %d]; got %d" % (MAX_K, self.k))
        self.rows, self.index = None, None             # the fitted rows (mu, ls) and their index, for predict
        self.f = None                                  # the two buffers; f[cur] holds the current iterate
        self.label_distributions_ = self.transduction_ = self.confidence_ = None
        self.n_iter_, self.converged_, self.delta_, self.n_unreached_ = 0, False, None, None

    # ---- the state ----
    def prepare_graph(self, rowptr, col, val, y):
        """takes any square CSR graph (symmetric for scikit-learn's meaning) and the labels y int64 [N] (outside [0, K): unlabelled)"""
        rowptr, col, val = _csr("LabelPropagator.prepare_graph", rowptr, col, val)
        self.rows, self.index = None, None             # (a graph of the caller's has no rows to search: predict is refused)
        n = rowptr.shape[0] - 1
        y = _labels("LabelPropagator.prepare_graph", y, n)
        dev = rowptr.device
        self.n, self.nnz = n, col.shape[0]
        self.rowptr, self.col, self.val = rowptr, col, val
        self.sval, self.deg = normalize_graph(rowptr, col, val, "sym" if self.variant == "spreading" else "row")
        self.f = [torch.empty(n, self.k_classes, dtype=torch.float32, device=dev) for _ in range(2)]
        self.label = torch.empty(n, dtype=torch.int64, device=dev)
        self.scratch = torch.empty(step_scratch(n, self.k_classes), dtype=torch.float64, device=dev)
        self.stats = torch.zeros(2, dtype=torch.float64, device=dev)
        self.label_distributions_ = self.transduction_ = self.confidence_ = None
        return self.reset(y)

    def prepare(self, mu, ls, y):
        """the k-NN graph of the posteriors (mu, ls) [N, dim] (knn_graph), then prepare_graph; keeps the rows for predict"""
        rowptr, col, val = knn_graph(mu, ls, self.k, self.metric, self.weights, self.perplexity)
        self.prepare_graph(rowptr, col, val, y)
        self.rows = (mu, ls)
        return self

    def reset(self, y=None):
        """the current buffer back to the one-hot labels (of y, if given: new labels for the same graph); device copies only"""
        if self.f is None:
            raise ValueError("LabelPropagator.reset: call prepare() or fit() first")
        if y is not None:
            self.label.copy_(_labels("LabelPropagator.reset", y, self.n))
        self.cur = 0
        labelled = (self.label >= 0) & (self.label < self.k_classes)
        hot = torch.arange(self.k_classes, device=self.label.device)[None, :] == self.label[:, None]
        self.f[0].copy_((hot & labelled[:, None]).float())
        self.n_iter_, self.converged_, self.delta_ = 0, False, None
        return self

    def step(self):
        """one iteration from the current buffer into the other -> stats float64 [2] on the device (rewritten by the next step):
        delta_l1 = sum |F_new - F_old| and delta_max"""
        if self.f is None:
            raise ValueError("LabelPropagator.step: call prepare() or fit() first")
        src, dst = self.f[self.cur], self.f[1 - self.cur]
        L.call("sv_lp_step", _p(src), self.n, _p(self.rowptr), _p(self.col) if self.nnz else None, _p(self.sval) if self.nnz else None,
               self.nnz, self.n, self.k_classes, _p(self.label), VARIANTS[self.variant], self.alpha, 1.0 - self.alpha, _p(dst),
               _p(self.scratch), _p(self.stats), _st())
        self.cur = 1 - self.cur
        return self.stats

    def _finish(self, f):
        n, dev = f.shape[0], f.device
        proba = torch.empty(n, self.k_classes, dtype=torch.float32, device=dev)
        pred = torch.empty(n, dtype=torch.int64, device=dev)
        conf = torch.empty(n, dtype=torch.float32, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        L.call("sv_lp_finish", _p(f), n, self.k_classes, _p(proba), _p(pred), _p(conf), _p(counts), _st())
        return proba, pred, conf, counts

    def finish(self):
        """label_distributions_, transduction_, confidence_ and counts_ (int64 [2] on the device: rows decided, rows unreached) of
        the current iterate (sv_lp_finish); no host read"""
        if self.f is None:
            raise ValueError("LabelPropagator.finish: call prepare() or fit() first")
        self.label_distributions_, self.transduction_, self.confidence_, self.counts_ = self._finish(self.f[self.cur])
        return self

    def fit(self, mu, ls, y, check_every=10):
        """prepare() and iterations until delta_l1 < tol -- scikit-learn's rule, read on the host once per `check_every` iterations
        (1: its n_iter_ exactly) -- or max_iter; then finish() and one more read for n_unreached_"""
        check_every = int(check_every)
        if check_every < 1:
            raise ValueError("LabelPropagator.fit: check_every must be >= 1")
        self.prepare(mu, ls, y)
        # (stats is read, where it is read, before the next step rewrites it: no copy per iteration)
        self.n_iter_, self.converged_, self.delta_ = _lp_loop(self.step, lambda stats: float(stats.cpu()[0]), self.max_iter, self.tol, check_every)
        self.finish()
        self.n_unreached_ = int(self.counts_.cpu()[1])
        return self

    # ---- out of sample ----
    def predict_proba(self, mu, ls=None):
        """scikit-learn's out-of-sample rule for a k-NN kernel: the mean of label_distributions_ over the query's k nearest FITTED rows
        (a fitted row finds itself), normalised -> fp32 [Q, K]; a bipartite CSR from LatentIndex.search, sv_lp_step's product
        variant, sv_lp_finish.  No host synchronisation."""
        return self._predict("LabelPropagator.predict_proba", mu, ls)[0]

    def predict(self, mu, ls=None):
        """-> the class of largest probability, int64 [Q] (the smaller index on a tie; -1 where no neighbour carries mass)"""
        return self._predict("LabelPropagator.predict", mu, ls)[1]

    def _predict(self, what, mu, ls):
        if self.label_distributions_ is None:
            raise ValueError("%s: no label distributions yet: call fit() or load_state_dict() first" % what)
        if self.rows is None:
            raise ValueError("%s: the propagator was fitted on a graph, not on rows: there is nothing to search" % what)
        dim = self.rows[0].shape[1]
        if not torch.is_tensor(mu) or mu.dim() != 2 or mu.shape[0] < 1 or mu.shape[1] != dim:
            raise ValueError("%s: mu must be a matrix [Q >= 1, %d]" % (what, dim))
        on_device(what, mu, ls, self.label_distributions_, *self.rows)
        if self.index is None:
            self.index = LatentIndex(dim, self.metric)
            self.index.add(*self.rows)
        n = len(self.index)
        k = min(self.k, n)
        idx = self.index.search(mu, ls, k=k)[1]
        q = mu.shape[0]
        rowptr = torch.arange(q + 1, dtype=torch.int64, device=mu.device) * k
        ones = torch.ones(q * k, dtype=torch.float32, device=mu.device)
        out = torch.empty(q, self.k_classes, dtype=torch.float32, device=mu.device)
        L.call("sv_lp_step", _p(self.label_distributions_), n, _p(rowptr), _p(idx), _p(ones), q * k, q, self.k_classes, None,
               L.LP_PRODUCT, 0.0, 0.0, _p(out), None, None, _st())
        proba, pred, _, _ = self._finish(out)
        return proba, pred

    # ---- checkpoints ----
    def state_dict(self):
        if self.label_distributions_ is None:
            raise ValueError("LabelPropagator.state_dict: nothing fitted yet")
        rows = None if self.rows is None else tuple(None if t is None else t.detach().clone() for t in self.rows)
        return dict(num_classes=self.k_classes, variant=self.variant, alpha=self.alpha, max_iter=self.max_iter, tol=self.tol, k=self.k,
                    metric=self.metric, weights=self.weights, perplexity=self.perplexity,
                    label_distributions=self.label_distributions_.clone(), transduction=self.transduction_.clone(),
                    mu=None if rows is None else rows[0], ls=None if rows is None else rows[1], n_iter=int(self.n_iter_),
                    converged=bool(self.converged_), delta=self.delta_, n_unreached=self.n_unreached_)

    def load_state_dict(self, state, device=None):
        """takes a state_dict() (tensors on any device; `device`: where to put them): the fitted distributions and the rows predict
        searches.  Nothing runs here: the first use refuses a propagator that is still on the host.  The graph and the iterates are not
        part of it: fit() starts anew."""
        if int(state["num_classes"]) != self.k_classes:
            raise ValueError("LabelPropagator.load_state_dict: the state has %d classes, the propagator %d"
                             % (int(state["num_classes"]), self.k_classes))
        dist, trans = state["label_distributions"], state["transduction"]
        if not torch.is_tensor(dist) or dist.dim() != 2 or dist.shape[1] != self.k_classes or not torch.is_tensor(trans) \
                or tuple(trans.shape) != (dist.shape[0],):
            raise ValueError("LabelPropagator.load_state_dict: label_distributions [N, %d] and transduction [N]" % self.k_classes)
        put = (lambda t: t.detach().contiguous().clone()) if device is None else (lambda t: t.detach().to(device).contiguous().clone())
        self.variant, self.alpha, self.k, self.metric = state["variant"], float(state["alpha"]), int(state["k"]), state["metric"]
        self.max_iter, self.tol, self.weights, self.perplexity = int(state["max_iter"]), float(state["tol"]), state["weights"], state["perplexity"]
        self.label_distributions_, self.transduction_ = put(dist.float()), put(trans.long())
        self.rows, self.index = None, None
        if state.get("mu") is not None:
            mu = put(state["mu"].float())
            if mu.dim() != 2 or mu.shape[0] != dist.shape[0]:
                raise ValueError("LabelPropagator.load_state_dict: mu must be a matrix of %d rows" % dist.shape[0])
            self.rows = (mu, None if state.get("ls") is None else put(state["ls"].float()))
        self.n_iter_, self.converged_ = int(state.get("n_iter", 0)), bool(state.get("converged", False))
        self.delta_, self.n_unreached_ = state.get("delta"), state.get("n_unreached")
        return self


def evaluate_propagation(model, fit_batches, test_batches=None, space="mu", labels_per_class=None, seed=0, mode="transductive",
                         chunk_rows=256, **args):
    """Graph-based semi-supervised classification on the codes of `model` (a VariationalAutoEncoder or a SmoothVAE, in eval mode:
    NotImplementedError otherwise): a LabelPropagator(classes, **args: its arguments, and fit's check_every) per label budget over the
    rows of fit_batches -- (image, label) tuples on the device.  space: "mu", the posteriors (mu, log sigma), or "features",
    model.features() where the model has it (metric "euclid" is then the default).  The images are regrouped into batches of
    chunk_rows rows before the model sees them (the encoders' last bits depend on the batch size) and all rows are gathered first:
    the result does not depend on the batching.  labels_per_class: None (all labels), a budget m, or a list of budgets, as in
    evaluate_probe (select_labels under ONE permutation drawn from `seed`).  mode="transductive": the rows of test_batches join the
    graph unlabelled; "inductive": the graph holds the fit rows and the test rows go through predict.  -> a dict budget -> dict:

        n_labelled                   the fit rows that kept a label
        accuracy_unlabelled          over the fit rows WITHOUT a label (NaN if there is none)
        accuracy_test                over the test rows (NaN without test_batches)
        n_unreached                  the graph's rows no label reached;   n_iter, converged   of the fit;   propagator

    Beyond fit's host reads, one host read per budget."""
    latent_family("evaluate_propagation", model)
    if space not in ("mu", "features"):
        raise ValueError("evaluate_propagation: space must be 'mu' or 'features'")
    if mode not in ("transductive", "inductive"):
        raise ValueError("evaluate_propagation: mode must be 'transductive' or 'inductive'")
    if space == "features" and not hasattr(model, "features"):
        raise ValueError("evaluate_propagation: %s has no features(): use space='mu'" % type(model).__name__)
    eval_only("evaluate_propagation", model)
    if chunk_rows is not None and int(chunk_rows) < 1:
        raise ValueError("evaluate_propagation: chunk_rows must be >= 1 or None")
    budgets = label_budgets("evaluate_propagation", labels_per_class)
    if mode == "inductive" and test_batches is None:
        raise ValueError("evaluate_propagation: mode='inductive' needs test_batches")
    check_every = args.pop("check_every", 10)
    if space == "features":
        args.setdefault("metric", "euclid")
    classes = num_classes(model)

    x_fit, ls_fit, y_fit = gather_codes("evaluate_propagation", model, fit_batches, space, chunk_rows)
    n_fit = x_fit.shape[0]
    if test_batches is not None:
        x_test, ls_test, y_test = gather_codes("evaluate_propagation", model, test_batches, space, chunk_rows)
    if args.get("metric", "kl") in ("euclid", "euclidean"):
        ls_fit = ls_test = None
    if mode == "transductive" and test_batches is not None:
        x_all = torch.cat([x_fit, x_test])
        ls_all = None if ls_fit is None else torch.cat([ls_fit, ls_test])
    else:
        x_all, ls_all = x_fit, ls_fit
    res = {}
    nan = torch.full((), float("nan"), dtype=torch.float64, device=x_fit.device)
    for m in budgets:
        y = y_fit if m is None else select_labels(y_fit, int(m), classes, seed)
        y_all = torch.cat([y, torch.full((x_all.shape[0] - n_fit,), -1, dtype=torch.int64, device=y.device)])
        lp = LabelPropagator(classes, **args).fit(x_all, ls_all, y_all, check_every=check_every)
        labelled = (y >= 0) & (y < classes)
        hidden = ~labelled & (y_fit >= 0) & (y_fit < classes)
        acc_u = ((lp.transduction_[:n_fit] == y_fit) & hidden).double().sum() / hidden.double().sum()       # (0 / 0: NaN)
        if test_batches is None:
            acc_t = nan
        else:
            pred = lp.transduction_[n_fit:] if mode == "transductive" else lp.predict(x_test, ls_test)
            acc_t = (pred == y_test).double().mean()
        host = torch.stack([labelled.double().sum(), acc_u, acc_t]).cpu().tolist()
        res[m] = dict(n_labelled=int(round(host[0])), accuracy_unlabelled=host[1], accuracy_test=host[2], n_unreached=lp.n_unreached_,
                      n_iter=lp.n_iter_, converged=lp.converged_, propagator=lp)
    return res
