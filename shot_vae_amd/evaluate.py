"""The evaluation pass of the reference loop -- valid() / test() of main_shot_vae.py:409-458 / :461-510 (the two bodies
are identical up to the TensorBoard tag) -- on the HIP path: eval-mode forward (BatchNorm with running statistics, the
sampler still stochastic: vae.py:37), the ELBO terms, the reported reconstruction metric MSE(sigmoid(rec), x) / (2 B
sigma^2) (always MSE, whatever --br says: :427-429), `ELBO` = mse + 0.01 (KL_c + KL_d) (:435), top-1 / top-5 from
disc_log_alpha (:441-447).

Every per-batch quantity stays on the device (the reference calls float() five times per batch = five host syncs);
`Evaluator.result()` does the one device-to-host copy of an epoch."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L


def _p(t):
    return C.c_void_p(t.data_ptr())


class Evaluator:
    """Running means of valid() / test() (lib/utils/avgmeter.py semantics: batch means weighted by batch size).

        ev = Evaluator(model, elbo_criterion)
        for image, label in loader: ev.update(image, label)
        top1, top5 = ev.result()["top1"], ev.result()["top5"]"""

    KEYS = ("klc", "kld", "mse", "elbo")

    def __init__(self, model, elbo_criterion, topk=5):
        self.model, self.crit, self.topk = model, elbo_criterion, topk
        self.reset()

    def reset(self):
        self.acc = None          # device: [sum klc*B, sum kld*B, sum mse*B, sum elbo*B, top1 hits, topk hits]
        self.count = 0

    def update(self, image, label):
        model, crit = self.model, self.crit
        if not image.is_cuda:
            raise L.ShotVaeHipError("Evaluator: inputs must be on an MI355X (no CPU fallback)")
        image = image.float().contiguous()
        label = label.long().contiguous()
        B = image.size(0)
        was_training = model.training
        model.eval()                                                     # :414
        try:
            with torch.no_grad():
                rec, mu, ls, la, *_ = model(image)                       # :423-424
                mu, ls, la = mu.contiguous(), ls.contiguous(), la.contiguous()
                out = torch.zeros(3, dtype=torch.float32, device=image.device)
                # MSE(sigmoid(rec), x) / (2 B sigma^2) + the two KL terms in one fused reduction (bce = 0): :425-429
                L.call("sv_elbo_fwd", _p(image), _p(rec.contiguous()), image[0].numel(), _p(mu), _p(ls), _p(la), B,
                       mu.shape[1], la.shape[1], 0, float(crit.x_sigma), _p(out),
                       C.c_void_p(torch.cuda.current_stream().cuda_stream))
                if self.acc is None:
                    self.acc = torch.zeros(6, dtype=torch.float32, device=image.device)
                mse, klc, kld = out[0], out[1], out[2]
                self.acc[:4] += B * torch.stack([klc, kld, mse, mse + 0.01 * (klc + kld)])        # :430-435
                L.call("sv_topk_hits", _p(la), _p(label), B, la.shape[1], self.topk, _p(self.acc[4:]),
                       C.c_void_p(torch.cuda.current_stream().cuda_stream))                       # :441-447
        finally:
            model.train(was_training)
        self.count += B
        return out

    def result(self):
        """dict(klc, kld, mse, elbo, top1, top5) as Python floats (one host sync)."""
        if self.acc is None or self.count == 0:
            return dict(klc=0.0, kld=0.0, mse=0.0, elbo=0.0, top1=0.0, top5=0.0)
        a = (self.acc / self.count).tolist()
        return dict(klc=a[0], kld=a[1], mse=a[2], elbo=a[3], top1=a[4], top5=a[5])


def evaluate(model, elbo_criterion, batches, topk=5):
    """valid() / test(): `batches` yields (image, label) device tensors; returns the result dict.  The reference returns
    (top1, top5) (:458)."""
    ev = Evaluator(model, elbo_criterion, topk)
    for image, label in batches:
        ev.update(image, label)
    return ev.result()


class SmoothEvaluator:
    """Test accuracy of a smooth-ELBO model (SmoothVAE), Trainer.eval of main_smooth_ELBO_svhn.py:217-226: the number of images
    whose predicted class (first maximum of alpha) is the label, over the number of images.  The two counters -- int64 [2] (hits,
    images) and the confusion matrix int64 [Dd, Dd], rows = labels -- live on the device and are added to by SmoothVAE.classify
    (sv_smooth_classify): update() never synchronises (the reference reads every batch back with .cpu().numpy()); result() does
    the one copy.  The module's mode is not touched: the encoder has no mode-dependent layer.

        ev = SmoothEvaluator(model)
        for image, label in loader: ev.update(image, label)
        accuracy = ev.result()["accuracy"]"""

    def __init__(self, model):
        self.model = model
        self.reset()

    def reset(self):
        self.counts = self.confusion = None

    def update(self, image, label):
        """adds one batch; returns its predictions (int64 [B], on the device)"""
        if not image.is_cuda or not label.is_cuda:
            raise L.ShotVaeHipError("SmoothEvaluator: inputs must be on an MI355X (no CPU fallback)")
        if self.counts is None:
            Dd = self.model.latent_disc_dim
            self.counts = torch.zeros(2, dtype=torch.int64, device=image.device)
            self.confusion = torch.zeros(Dd, Dd, dtype=torch.int64, device=image.device)
        return self.model.classify(image, label.long(), self.counts, self.confusion)[1]

    def result(self):
        """dict(accuracy = correct / total (0.0 before any update), correct, total, per_class_accuracy, confusion): Python numbers,
        and numpy arrays for the last two -- confusion int64 [Dd, Dd] with confusion[label][pred], per_class_accuracy float64 [Dd] =
        its diagonal over its row sums (NaN for a class without images).  A row without a prediction (NaN logits) or with a label
        outside [0, Dd) is a miss in `total` and is not in the matrix.  One host synchronisation."""
        if self.counts is None:
            return dict(accuracy=0.0, correct=0, total=0, per_class_accuracy=None, confusion=None)
        Dd = self.confusion.shape[0]
        flat = torch.cat([self.counts, self.confusion.view(-1)]).cpu().numpy()
        correct, total = int(flat[0]), int(flat[1])
        conf = flat[2:].reshape(Dd, Dd).copy()
        rows = conf.sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            per_class = np.where(rows > 0, np.diag(conf) / np.maximum(rows, 1), np.nan)
        return dict(accuracy=correct / total if total else 0.0, correct=correct, total=total, per_class_accuracy=per_class,
                    confusion=conf)


def evaluate_smooth(model, batches):
    """Trainer.eval over `batches` of (image, label) device pairs -> SmoothEvaluator.result().  Integer counts: the result does not
    depend on how the test set is batched (a ragged last batch included)."""
    ev = SmoothEvaluator(model)
    for image, label in batches:
        ev.update(image, label)
    return ev.result()


class KnnEvaluator:
    """k-NN accuracy of a model's latent space: every test image is encoded (neighbors.encode_posterior) and classified by the vote of
    its k nearest rows of `index` (a neighbors.LatentIndex built with num_classes over the labelled pool).  As in SmoothEvaluator the
    counters -- int64 [2] (hits, images) and the confusion matrix int64 [K, K], rows = labels -- live on the device and are added to
    by sv_knn_vote: update() never synchronises, result() does the one copy of a test set.

        ev = KnnEvaluator(model, index, k=20)
        for image, label in loader: ev.update(image, label)
        accuracy = ev.result()["accuracy"]"""

    def __init__(self, model, index, k=20, weights="uniform", tau=1.0):
        if index.num_classes is None:
            raise ValueError("KnnEvaluator: the index was built without num_classes")
        self.model, self.index, self.k, self.weights, self.tau = model, index, int(k), weights, float(tau)
        self.reset()

    def reset(self):
        self.counts = self.confusion = None

    def update(self, image, label):
        """adds one batch; returns its predictions (int64 [B], on the device)"""
        if not image.is_cuda or not label.is_cuda:
            raise L.ShotVaeHipError("KnnEvaluator: inputs must be on an MI355X (no CPU fallback)")
        from .neighbors import encode_posterior
        mu, ls = encode_posterior(self.model, image)
        if self.counts is None:
            K = self.index.num_classes
            self.counts = torch.zeros(2, dtype=torch.int64, device=image.device)
            self.confusion = torch.zeros(K, K, dtype=torch.int64, device=image.device)
        return self.index.classify(mu, ls, self.k, weights=self.weights, tau=self.tau, label=label.long(), counts=self.counts,
                                   confusion=self.confusion)

    result = SmoothEvaluator.result      # the same counters, the same read-out: accuracy, correct, total, per_class_accuracy, confusion


def evaluate_knn(model, gallery_batches, test_batches, k=20, metric="kl", weights="uniform", tau=1.0, num_classes=None):
    """Top-1 k-NN accuracy of the latent space: the posteriors of `gallery_batches` ((image, label) device pairs: the labelled pool)
    are the gallery, every image of `test_batches` votes among its k nearest under `metric` -> KnnEvaluator.result(): accuracy,
    correct, total, per_class_accuracy, confusion.  num_classes defaults to the model's number of classes.  The model must be in eval
    mode (encode_posterior).  Integer counts: the result does not depend on how either set is batched."""
    from .neighbors import LatentIndex, encode_posterior, metric_code
    metric_code(metric)                                                     # an unknown metric fails before any encoding
    if num_classes is None:
        num_classes = model.latent_disc_dim if hasattr(model, "latent_disc_dim") else model._plan.K
    index = None
    for image, label in gallery_batches:
        mu, ls = encode_posterior(model, image)
        if index is None:
            index = LatentIndex(mu.shape[1], metric=metric, num_classes=num_classes)
        index.add(mu, ls, label)
    if index is None:
        raise ValueError("evaluate_knn: the gallery is empty")
    ev = KnnEvaluator(model, index, k, weights, tau)
    for image, label in test_batches:
        ev.update(image, label)
    return ev.result()


def evaluate_scores(model, criterion, batches, samples=0, key=None):
    """Dataset means of the per-image scores (VariationalAutoEncoder.score_terms): dict(elbo, recon, kl_c, kl_d) at
    z = mu with samples=0, and with samples > 0 (key: an int or a 1-element int64 device tensor) the same terms over `samples` posterior
    draws plus log_px and bits_per_dim = -log_px / (D ln 2), D = the elements of one image.  `batches` yields image tensors or
    (image, ...) tuples on the device.  The model must be in eval mode, as for score() (NotImplementedError otherwise: nothing here
    switches it), and the dataset must not be empty (ValueError).  An image's draws are indexed by its position in the dataset
    (row0 = the running image count), so the result does not depend on how the dataset was batched; the sums stay on the device
    (float64) until the one copy at the end."""
    samples = int(samples)
    if samples < 0:
        raise ValueError("evaluate_scores: samples must be >= 0")
    if samples > 0 and key is None:
        raise ValueError("evaluate_scores: samples > 0 needs a key")
    want = ("elbo", "recon", "kl_c", "kl_d") + (("log_px",) if samples > 0 else ())
    acc, count, dim = None, 0, 0
    for batch in batches:
        image = batch[0] if isinstance(batch, (tuple, list)) else batch
        if samples > 0 and isinstance(key, int) and not isinstance(key, bool) and image.is_cuda:
            key = torch.tensor([key], dtype=torch.int64, device=image.device)         # one copy for the whole dataset
        out = model.score_terms(image, criterion, want, samples=max(samples, 1), key=key if samples > 0 else None, row0=count,
                                what="evaluate_scores")
        sums = torch.stack([out[w].double().sum() for w in want])
        acc = sums if acc is None else acc + sums
        count += image.size(0)
        dim = image[0].numel()
    if acc is None:
        raise ValueError("evaluate_scores: the dataset is empty")
    res = dict(zip(want, (acc / count).tolist()))
    if samples > 0:
        res["bits_per_dim"] = -res["log_px"] / (dim * math.log(2.0))
    return res
