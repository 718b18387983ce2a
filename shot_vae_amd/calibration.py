"""How far can the class posterior q(y | x) be trusted, and does a score separate two sets of images?  Calibration, temperature scaling and
detection metrics on the HIP path (csrc/calib.hip).

    rel = Reliability(10)
    for image, label in loader:
        rel.update(model.encode(image)[2], label)                       # logits; kind="prob" for a smooth model's alpha
    rel.result()                                                        # accuracy, ece, mce, nll, brier, entropy, the diagram

    ts = TemperatureScaler().fit(val_logits, val_label)                 # Newton steps on the device; ts.temperature: a device float
    row_stats(test_logits, test_label, temperature=ts.temperature)

    detection_metrics(score, positive)                                  # auroc, aupr, aupr_neg, fpr_at_tpr: device scalars
    selective_metrics(conf, correct)                                    # aurc, e_aurc
    evaluate_calibration(model, loader)                                 # the three model families
    evaluate_detection(model, in_loader, out_loader, score="msp")

A posterior is given as logits / log-probabilities (kind "logit": SHOT-VAE's log_alpha, the classifier's logits) or as probabilities
(kind "prob": the smooth-ELBO models' alpha).  There is no float atomic -- the same call sequence gives the same bits --, nothing here
synchronises with the host except where stated, and there is no CPU fallback."""
import collections

import torch

from . import _lib as L
from .aggregate import partials
from ._latent import _p, _st, eval_only, on_device, regroup, split_batch, vectors

KINDS = {"logit": L.CAL_LOGIT, "prob": L.CAL_PROB}
MAX_BINS = 1024               # sv_calib_accum: the histogram of a block lives in LDS

RowStats = collections.namedtuple("RowStats", "pred conf nll brier entropy")
CalibrationResult = collections.namedtuple(
    "CalibrationResult", "accuracy confidence ece mce nll brier entropy n bin_accuracy bin_confidence bin_count edges")
DetectionResult = collections.namedtuple("DetectionResult", "auroc aupr aupr_neg fpr_at_tpr")
SelectiveResult = collections.namedtuple("SelectiveResult", "aurc e_aurc")


def _kind(kind):
    if kind not in KINDS:
        raise ValueError("unknown kind %r (one of %s)" % (kind, ", ".join(sorted(KINDS))))
    return KINDS[kind]


def _posterior(what, x, label, need_label=False, classes=None):
    """x as a contiguous fp32 device matrix [n, k] and label as an int64 vector [n]; the shape checks come first (they need no device),
    then the no-CPU rule"""
    if not torch.is_tensor(x) or x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError("%s: x must be a non-empty matrix [n, classes]" % what)
    if classes is not None and x.shape[1] != classes:
        raise ValueError("%s: x has %d columns, not %d classes" % (what, x.shape[1], classes))
    if label is None:
        if need_label:
            raise ValueError("%s: the labels are required" % what)
    elif not torch.is_tensor(label) or label.is_floating_point() or label.numel() != x.shape[0]:
        raise ValueError("%s: label must be an integer vector [%d]" % (what, x.shape[0]))
    on_device(what, x, label)
    return x.detach().float().contiguous(), (label.reshape(-1).long().contiguous() if label is not None else None)


def _temperature(what, temperature, device=None):
    """None, or the temperature as sv_calib_rows reads it: a 1-element fp32 device tensor (a number is copied to `device`; without a
    device the value is only checked, which needs none)"""
    if temperature is None:
        return None
    if torch.is_tensor(temperature):
        if temperature.dtype != torch.float32 or temperature.numel() != 1:
            raise ValueError("%s: temperature must be a number or a 1-element fp32 device tensor" % what)
        if device is not None and not temperature.is_cuda:
            raise L.ShotVaeHipError("%s: temperature is not on an MI355X (no CPU fallback)" % what)
        return temperature.reshape(1)
    if not float(temperature) > 0:
        raise ValueError("%s: temperature must be > 0" % what)
    if device is None:
        return None
    return torch.tensor([float(temperature)], dtype=torch.float32, device=device)


def _rows_into(code, x, label, temp, pred, conf, nll, brier, entropy):
    L.call("sv_calib_rows", code, _p(x), x.shape[1], x.shape[0], x.shape[1], _p(temp), _p(label), _p(pred), _p(conf), _p(nll), _p(brier),
           _p(entropy), _st())


def row_stats(x, label=None, kind="logit", temperature=None):
    """-> RowStats(pred int64 [n], conf, nll, brier, entropy fp32 [n]) of the posteriors x [n, classes] on the device: the first maximum,
    its probability, -log p[label], sum_k (p_k - [k == label])^2 and -sum p log p of p = softmax(x / T) ("logit") or of p proportional to
    x^(1/T) ("prob").  temperature: a number, or a 1-element fp32 device tensor that is read on the device (a captured call follows a
    refitted temperature).  A row that is not finite gives pred = -1 and NaN; without a label (or with one outside [0, classes)) nll and
    brier are NaN.  No host synchronisation."""
    code = _kind(kind)
    _temperature("row_stats", temperature)
    x, label = _posterior("row_stats", x, label)
    temp = _temperature("row_stats", temperature, x.device)
    n, dev = x.shape[0], x.device
    out = RowStats(torch.empty(n, dtype=torch.int64, device=dev), *[torch.empty(n, dtype=torch.float32, device=dev) for _ in range(4)])
    _rows_into(code, x, label, temp, *out)
    return out


class Reliability:
    """The reliability histogram of a classifier over a whole set: accuracy and mean confidence per confidence bin, and from them the
    expected and the maximum calibration error, beside the mean NLL, Brier score and entropy.

    update() runs sv_calib_rows and appends the per-row values to doubling buffers (LatentIndex's scheme); it makes no host read and can
    be captured under torch.cuda.graph.  result() bins everything at once (sv_calib_accum, sv_calib_finish) and makes ONE host read: it
    does not depend on how the rows were batched, by construction.  Bins are (lo, hi] intervals of the confidence; a row whose label is
    outside [0, num_classes) or whose posterior is not finite is in no bin and in no mean."""

    FIELDS = (("conf", torch.float32), ("pred", torch.int64), ("label", torch.int64), ("nll", torch.float32), ("brier", torch.float32),
              ("entropy", torch.float32))

    def __init__(self, num_classes, bins=15, edges=None):
        self.num_classes = int(num_classes)
        if self.num_classes < 1:
            raise ValueError("Reliability: num_classes must be >= 1")
        if edges is not None:
            edges = torch.as_tensor(edges, dtype=torch.float64).reshape(-1)
            if edges.numel() < 2 or bool((edges[1:] < edges[:-1]).any()) or bool(torch.isnan(edges).any()):
                raise ValueError("Reliability: edges must be a non-decreasing vector of at least two values")
            bins = edges.numel() - 1
        self.bins = int(bins)
        if not 1 <= self.bins <= MAX_BINS:
            raise ValueError("Reliability: bins must be in [1, %d] (sv_calib_accum's histogram lives in LDS); got %d" % (MAX_BINS, self.bins))
        self.edges = (edges if edges is not None else torch.linspace(0.0, 1.0, self.bins + 1, dtype=torch.float64)).float()
        self.n = 0
        self.buf = None

    def __len__(self):
        return self.n

    def _grow(self, need, device):
        cap = 0 if self.buf is None else self.buf["conf"].shape[0]
        if need <= cap:
            return
        new = max(need, 2 * cap, 1024)
        grown = {name: torch.empty(new, dtype=dt, device=device) for name, dt in self.FIELDS}
        if self.buf is not None:
            for name, _ in self.FIELDS:
                grown[name][:self.n] = self.buf[name][:self.n]
        self.buf = grown

    def reserve(self, rows, device):
        """room for `rows` rows in all: an update() that fits allocates nothing (a captured update must fit)"""
        self._grow(int(rows), device)
        return self

    def update(self, x, label, kind="logit", temperature=None):
        """appends the rows of the posteriors x [n, num_classes] with their labels [n]; returns the index of the first row added"""
        code = _kind(kind)
        _temperature("Reliability.update", temperature)
        x, label = _posterior("Reliability.update", x, label, need_label=True, classes=self.num_classes)
        temp = _temperature("Reliability.update", temperature, x.device)
        n, first = x.shape[0], self.n
        self._grow(first + n, x.device)
        b = {name: t[first:first + n] for name, t in self.buf.items()}
        b["label"].copy_(label)
        _rows_into(code, x, label, temp, b["pred"], b["conf"], b["nll"], b["brier"], b["entropy"])
        self.n += n
        return first

    def _adaptive_edges(self, conf, valid):
        """equal-mass inner edges from ONE sort of the valid confidences: edge i is the largest of the floor(i n / B) smallest
        values, so the bins' counts differ by one at most (ties aside); nothing here depends on n on the host"""
        B = self.bins
        ordered = torch.sort(torch.where(valid, conf, torch.full_like(conf, float("inf"))))[0]
        n = valid.sum()
        upto = torch.arange(1, B, device=conf.device, dtype=torch.int64) * n // B            # rows below inner edge i
        inner = torch.where(upto > 0, ordered[(upto - 1).clamp(min=0)], torch.full((B - 1,), float("-inf"), device=conf.device))
        edges = torch.empty(B + 1, dtype=torch.float32, device=conf.device)
        edges[0], edges[B] = 0.0, 1.0
        edges[1:B] = inner
        return edges

    def reduce(self, adaptive=False):
        """result() without its host read -> device tensors (out fp32 [8 + 2 bins]: sv_calib_finish's out, then its diagram; ints int64
        [2 bins + 3]: bin_count, bin_correct, counts; edges fp32 [bins + 1]).  Capturable."""
        if self.n < 1:
            raise ValueError("Reliability.result: no rows yet")
        b = {name: t[:self.n] for name, t in self.buf.items()}
        dev, B, K = b["conf"].device, self.bins, self.num_classes
        if adaptive:
            edges = self._adaptive_edges(b["conf"], (b["pred"] >= 0) & (b["label"] >= 0) & (b["label"] < K))
        else:
            edges = self.edges = self.edges.to(dev)
        P = partials(1, self.n)
        ints = torch.zeros(2 * B + 3, dtype=torch.int64, device=dev)
        sums = torch.empty(P, B + 3, dtype=torch.float64, device=dev)
        out = torch.empty(8 + 2 * B, dtype=torch.float32, device=dev)
        L.call("sv_calib_accum", _p(b["conf"]), _p(b["pred"]), _p(b["label"]), _p(b["nll"]), _p(b["brier"]), _p(b["entropy"]), self.n, K,
               _p(edges), B, _p(ints[:B]), _p(ints[B:]), _p(ints[2 * B:]), _p(sums), P, 1, _st())
        L.call("sv_calib_finish", _p(ints[:B]), _p(ints[B:]), _p(ints[2 * B:]), _p(sums), P, B, _p(out[:8]), _p(out[8:]), _st())
        return out, ints, edges

    def result(self, adaptive=False):
        """-> CalibrationResult: accuracy, confidence (its mean), ece = sum_b n_b / n |acc_b - conf_b|, mce = the largest gap of a
        non-empty bin, the means of nll, brier and entropy, n (the valid rows) -- Python floats --, and bin_accuracy, bin_confidence
        (fp32 [bins], NaN for an empty bin), bin_count (int64 [bins]), edges (fp32 [bins + 1]) as host tensors.  adaptive: equal-mass
        bins of the rows seen instead of the edges given.  ONE host read."""
        out, ints, edges = self.reduce(adaptive)
        B = self.bins
        host = torch.cat([out.double(), ints[:B].double(), edges.double()]).cpu()          # (a count is exact in a double)
        o = host[:8].tolist()
        return CalibrationResult(*o[:7], int(o[7]), host[8:8 + B].float(), host[8 + B:8 + 2 * B].float(),
                                 host[8 + 2 * B:8 + 3 * B].long(), host[8 + 3 * B:].float())


class TemperatureScaler:
    """Temperature scaling (Guo et al. 2017): the T > 0 that minimises the NLL of softmax(x / T) on a labelled validation split, found
    by Newton's method on beta = 1 / T, in which the NLL is convex.  One iteration = sv_temp_accum + sv_temp_update, two launches and no
    host read; a step is clamped to [beta / 4, 4 beta].  step() can be captured under torch.cuda.graph; `.temperature` is the 1-element
    fp32 device tensor every other call here accepts, `.beta` its float64 inverse, `.stats` the last update's fp32 [4]: the mean NLL at
    the beta the step started from, the mean gradient, the step, the new beta."""

    def __init__(self, kind="logit"):
        self.kind, self.code = kind, _kind(kind)
        self.temperature = self.beta = self.stats = None

    def reset(self, device, temperature=1.0):
        if not float(temperature) > 0:
            raise ValueError("TemperatureScaler.reset: temperature must be > 0")
        self.beta = torch.tensor([1.0 / float(temperature)], dtype=torch.float64, device=device)
        self.temperature = torch.tensor([float(temperature)], dtype=torch.float32, device=device)
        self.stats = torch.full((4,), float("nan"), dtype=torch.float32, device=device)
        return self

    def step(self, x, label):
        """one Newton iteration on the rows (x [n, classes], label [n]) from the current temperature, in place -> stats"""
        x, label = _posterior("TemperatureScaler.step", x, label, need_label=True)
        if self.beta is None:
            self.reset(x.device)
        n, K = x.shape
        P = partials(1, n)
        sums = torch.empty(P, 3, dtype=torch.float64, device=x.device)
        count = torch.empty(P, dtype=torch.int64, device=x.device)
        L.call("sv_temp_accum", self.code, _p(x), K, n, K, _p(label), _p(self.beta), _p(sums), _p(count), P, 1, _st())
        L.call("sv_temp_update", _p(sums), _p(count), P, _p(self.beta), _p(self.temperature), _p(self.stats), _st())
        return self.stats

    def fit(self, x, label, iters=12, temperature=1.0):
        """`iters` Newton iterations from `temperature`; reads stats ONCE at the end: self.nll = the mean NLL the last iteration
        started from, self.last_step = its step in beta (how far from converged)"""
        iters = int(iters)
        if iters < 1:
            raise ValueError("TemperatureScaler.fit: iters must be >= 1")
        x, label = _posterior("TemperatureScaler.fit", x, label, need_label=True)
        self.reset(x.device, temperature)
        for _ in range(iters):
            self.step(x, label)
        host = self.stats.cpu()
        self.nll, self.last_step = float(host[0]), float(host[2])
        return self


def rank_counts(q, g, weight=None):
    """-> (greater, equal) int64 [len(q)] on the device: the (weighted) number of values of g above, and equal to, every q[i]
    (sv_rank_scan: exact, the [len(q), len(g)] matrix is never stored).  weight: int64 [len(g)], non-negative -- a MASK keeps every
    shape independent of the data.  A NaN on either side counts nowhere; -0 == 0.  No host synchronisation."""
    if torch.is_tensor(weight) and weight.is_floating_point():
        raise ValueError("rank_counts: weight must be an integer vector")
    g, weight = vectors("rank_counts (g, weight)", g, weight)
    q, g = vectors("rank_counts (q)", q)[0].float().contiguous(), g.float().contiguous()
    if weight is not None:
        weight = weight.long().contiguous()
    Q, N = q.numel(), g.numel()
    out = torch.zeros(2, Q, dtype=torch.int64, device=q.device)
    L.call("sv_rank_scan", _p(q), Q, _p(g), _p(weight), N, partials(-(-Q // 256), -(-N // 16)), _p(out[0]), _p(out[1]), _st())
    return out[0], out[1]


def detection_metrics(score, positive, tpr=0.95):
    """How well does `score` (fp32 [n]; HIGHER means more positive) separate the rows with positive != 0 from the others?  From two
    scans of the scores against themselves, weighted by the positives and by the negatives (TP>=, FP>= = the positives / negatives
    scoring at least as high as row i):

        auroc       sum over the positives of (N_neg - greater - equal / 2) / (N_pos N_neg): the Mann-Whitney statistic, ties count half
        aupr        the mean over the positives of TP>= / (TP>= + FP>=): scikit-learn's average_precision_score, ties grouped
        aupr_neg    the same for the negatives under the negated score
        fpr_at_tpr  the least FP>= / N_neg over the positives with TP>= / N_pos >= tpr (the ratio is formed as roc_curve forms it, so
                    that 95 of 100 meets 0.95)

    -> DetectionResult of float64 device scalars; no host synchronisation.  A row with a NaN score is left out.  Without a positive or
    without a negative row the ratios are NaN."""
    if not 0.0 < float(tpr) <= 1.0:
        raise ValueError("detection_metrics: tpr must be in (0, 1]")
    score, positive = vectors("detection_metrics (score, positive)", score, positive)
    score = score.float().contiguous()
    seen = ~torch.isnan(score)
    pos = (positive != 0) & seen
    neg = (positive == 0) & seen
    gp, ep = rank_counts(score, score, pos.long())
    gn, en = rank_counts(score, score, neg.long())
    n_pos, n_neg = pos.sum().double(), neg.sum().double()
    tp, fp = (gp + ep).double(), (gn + en).double()
    zero = torch.zeros_like(tp)
    auroc = torch.where(pos, n_neg - gn.double() - 0.5 * en.double(), zero).sum() / (n_pos * n_neg)
    aupr = torch.where(pos, tp / (tp + fp), zero).sum() / n_pos
    # under the negated score a row's "at least as high" are the rows scoring at most as high: everything but the greater ones
    tn_le, fn_le = neg.sum() - gn, pos.sum() - gp
    aupr_neg = torch.where(neg, tn_le.double() / (tn_le + fn_le).double(), zero).sum() / n_neg
    reach = pos & (tp / n_pos >= float(tpr))
    fpr = torch.where(reach, fp / n_neg, torch.full_like(tp, float("inf"))).min()
    fpr = torch.where(torch.isinf(fpr), torch.full_like(fpr, float("nan")), fpr)
    return DetectionResult(auroc, aupr, aupr_neg, fpr)


def selective_metrics(conf, correct):
    """Selective prediction: answer only the rows whose confidence is high enough.  With n_i the rows and e_i the errors (correct == 0)
    at confidence >= conf_i:

        aurc    the mean over the rows of the selective risk e_i / n_i (Geifman & El-Yaniv 2017).  Rows of EQUAL confidence share their
                group's risk -- no order among them is invented --, so on tie-free data this is the sorted cumulative formulation
        e_aurc  aurc minus the least value any confidence could reach with the same n rows and e errors (every error ranked last),
                computed from the integers: sum_{i > n - e} (i - (n - e)) / i / n

    -> SelectiveResult of float64 device scalars; no host synchronisation.  A NaN confidence ranks nowhere (and its own risk is NaN)."""
    conf, correct = vectors("selective_metrics (conf, correct)", conf, correct)
    conf = conf.float().contiguous()
    wrong = (correct == 0).long()
    g, e = rank_counts(conf, conf)
    gw, ew = rank_counts(conf, conf, wrong)
    n = conf.numel()
    aurc = ((gw + ew).double() / (g + e).double()).mean()
    i = torch.arange(1, n + 1, device=conf.device, dtype=torch.float64)
    best = ((i - (n - wrong.sum()).double()).clamp(min=0.0) / i).sum() / n
    return SelectiveResult(aurc, aurc - best)


def _family(what, model):
    """-> (family name, image -> (class posterior, its kind)) for the three model families"""
    from .classifier import WideResNetClassifier
    from .smooth import SmoothVAE
    from .vae import VariationalAutoEncoder
    if isinstance(model, VariationalAutoEncoder):
        return "shot", lambda image: (model.encode(image)[2], "logit")
    if isinstance(model, SmoothVAE):
        return "smooth", lambda image: (model.classify(image)[0], "prob")
    if isinstance(model, WideResNetClassifier):
        def logits(image):
            with torch.no_grad():
                return model(image), "logit"
        return "classifier", logits
    raise TypeError("%s: a VariationalAutoEncoder, a SmoothVAE or a WideResNetClassifier, not %s" % (what, type(model).__name__))


def evaluate_calibration(model, batches, bins=15, adaptive=False, temperature=None, chunk_rows=256):
    """The calibration of `model`'s class posterior over `batches` ((image, label) batches on the device): SHOT-VAE's log_alpha
    (encode), a smooth-ELBO model's alpha (classify) or the classifier's logits -> Reliability(...).result(adaptive) of all rows, under
    `temperature` if given.  Eval mode only.  The images are regrouped into batches of chunk_rows rows before the model sees them (the
    encoders' last bits depend on the batch size): the result does not depend on how the caller batched the set, only on the order of
    its rows.  chunk_rows=None takes the batches as they come.  One host read at the end."""
    _, posterior = _family("evaluate_calibration", model)
    eval_only("evaluate_calibration", model)
    if chunk_rows is not None and int(chunk_rows) < 1:
        raise ValueError("evaluate_calibration: chunk_rows must be >= 1 or None")
    rel = None
    for image, label in regroup("evaluate_calibration", batches, None if chunk_rows is None else int(chunk_rows)):
        x, kind = posterior(image)
        if rel is None:
            rel = Reliability(x.shape[1], bins=bins)
        rel.update(x, label, kind=kind, temperature=temperature)
    if rel is None:
        raise ValueError("evaluate_calibration: the dataset is empty")
    return rel.result(adaptive=adaptive)


SCORES = ("msp", "entropy", "elbo", "log_px", "mixture")


def evaluate_detection(model, in_batches, out_batches, score="msp", criterion=None, tpr=0.95, mixture=None, **score_args):
    """Out-of-distribution detection: does a per-image score of `model` separate the images of in_batches (the POSITIVE class) from
    those of out_batches (batches of images, or (image, ...) tuples, on the device)?

        "msp"      the maximum class probability (Hendrycks & Gimpel 2017)          "entropy"   minus the posterior's entropy
        "elbo"     SHOT-VAE's per-image ELBO                                        "log_px"    its importance-weighted log-likelihood
        "mixture"  the log-density of the image's posterior mean under `mixture`, a mixture.GaussianMixture fitted to the codes of
                   in-distribution data: one encoder pass, no decoder (a VariationalAutoEncoder or a SmoothVAE)

    The last two exist for a VariationalAutoEncoder only (score_terms with `criterion` and **score_args: samples, key, ...); for the
    other families they are refused with a ValueError before anything runs.  -> detection_metrics of all rows.  Eval mode only; no host
    synchronisation."""
    if score not in SCORES:
        raise ValueError("evaluate_detection: score must be one of %s" % ", ".join(SCORES))
    family, posterior = _family("evaluate_detection", model)
    if (score == "mixture") != (mixture is not None):
        raise ValueError("evaluate_detection: score 'mixture' needs a fitted mixture, and only that score takes one")
    if score == "mixture" and family == "classifier":
        raise ValueError("evaluate_detection: score 'mixture' needs a latent code: a VariationalAutoEncoder or a SmoothVAE")
    if score in ("elbo", "log_px"):
        if family != "shot":
            raise ValueError("evaluate_detection: score %r needs a decoder with a per-image likelihood: a VariationalAutoEncoder, not %s"
                             % (score, type(model).__name__))
        if criterion is None:
            raise ValueError("evaluate_detection: score %r needs the criterion (its reconstruction mode and x_sigma)" % score)
    elif criterion is not None or score_args:
        raise ValueError("evaluate_detection: score %r takes no criterion and no score arguments" % score)
    eval_only("evaluate_detection", model)
    values, positive = [], []
    for flag, batches in ((1, in_batches), (0, out_batches)):
        seen = 0
        for batch in batches:
            image = split_batch("evaluate_detection", batch, None)[0]
            if score in ("elbo", "log_px"):
                args = dict(score_args)
                if "row0" not in args and args.get("key") is not None:
                    args["row0"] = seen                     # every image its own draws, whatever the batching
                v = model.score_terms(image, criterion, (score,), what="evaluate_detection", **args)[score]
            elif score == "mixture":
                from .neighbors import encode_posterior
                v = mixture.score_samples(encode_posterior(model, image)[0])
            else:
                x, kind = posterior(image)
                stats = row_stats(x, kind=kind)
                v = stats.conf if score == "msp" else -stats.entropy
            values.append(v)
            positive.append(torch.full((v.numel(),), flag, dtype=torch.int64, device=v.device))
            seen += v.numel()
        if not seen:
            raise ValueError("evaluate_detection: %s is empty" % ("in_batches" if flag else "out_batches"))
    return detection_metrics(torch.cat(values), torch.cat(positive), tpr=tpr)
