"""The supervised baseline of the reference -- ``classifier_model.wideresnet.WideResNet`` / ``get_wide_resnet``
(classifier_model/wideresnet.py:68-141), ``nn.CrossEntropyLoss()`` and the loop bodies of main_classifier.py (train :189-198,
test :213-277) -- on the HIP path.

The encoder is the SHOT-VAE's (the two wideresnet.py files are identical down to the units); behind the pool sits one
Linear(C, num_classes) that returns raw logits (sv_fc_fwd / sv_fc_bwd), the loss is a row-wise stable log-sum-exp (sv_ce_fwd /
sv_ce_bwd).  Same state_dict keys as the reference in both ``data_parallel`` layouts, same flat parameter / gradient buffers as
VariationalAutoEncoder (FlatSGD, dp.all_reduce_gradients work on it unchanged).
"""
import ctypes as C
import re

import torch
from torch import nn

from . import _lib as L
from .engine import Plan
from .train import GraphedStep, apply_update
from .vae import FlatModule, check_drop_rate


def _p(t):
    return C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _ClassifierFunction(torch.autograd.Function):
    """One autograd node for the whole network, as _VAEFunction is for the VAE."""

    @staticmethod
    def forward(ctx, anchor, model, image, keys):
        logits, f = model._engine.forward_classifier(image, model.training, keep=True, keys=keys)
        ctx.model, ctx.f = model, f
        return logits

    @staticmethod
    def backward(ctx, d_logits):
        model, f = ctx.model, ctx.f
        if f is None:
            raise RuntimeError("backward through the same classifier forward twice is not supported")
        if not f.training:
            raise NotImplementedError("backward through an eval-mode forward (BatchNorm with running statistics) is not "
                                      "implemented; the reference never does it (main_classifier.py:222-223: no_grad)")
        ctx.f = None
        model._attach_grads()
        model._engine.backward_classifier(f, d_logits)
        return (None,) * 4


class WideResNetClassifier(FlatModule):
    """Drop-in for classifier_model.wideresnet.WideResNet: same constructor keywords (plus compute_dtype and rng, as
    VariationalAutoEncoder), same forward signature, fp32 logits [B, num_classes]."""

    TOP_MODULES = ("encoder", "global_avg", "classification")

    def __init__(self, num_input_channels=3, num_init_features=16, depth=28, width=2, num_classes=10, data_parallel=True,
                 small_input=True, drop_rate=0.0, compute_dtype="bf16", rng="host"):
        super(WideResNetClassifier, self).__init__()
        assert (depth - 4) % 6 == 0, 'depth should be 6n+4'
        drop_rate = check_drop_rate(drop_rate)
        if not small_input:
            raise NotImplementedError("small_input=False (7x7 stem + max-pool) is not implemented; the CIFAR / SVHN configs of "
                                      "main_classifier.py use small_input=True")
        if num_init_features != 16:
            raise NotImplementedError("num_init_features=%s: the stem is built 16 channels wide (the reference's default, which "
                                      "get_wide_resnet never changes)" % (num_init_features,))
        if int(width) != width or int(depth) != depth:
            raise NotImplementedError("depth and width are integers (wideresnet-D-W); got %s, %s" % (depth, width))
        plan = Plan("wideresnet-%d-%d" % (depth, width), in_ch=num_input_channels, K=int(num_classes), drop_rate=drop_rate,
                    head="classifier")
        self._init_flat(plan, compute_dtype, data_parallel, rng, drop_rate)
        self._widths = list(plan.widths)
        self._engine.init_classifier()
        self._build_tree()

    def forward(self, input_img, mixup_alpha=None, label=None, manifold_mixup=False, mixup_layer_list=None):
        """logits of input_img; the other arguments are accepted and ignored, as the reference's forward ignores them
        (classifier_model/wideresnet.py:120-125)"""
        if not input_img.is_cuda:
            raise L.ShotVaeHipError("WideResNetClassifier: input is not on an MI355X (no CPU fallback)")
        keys = None
        if self._drop_active():
            keys = self._draw_keys(1, input_img.device)
            self._log_keys(keys)
        if torch.is_grad_enabled():
            if self._anchor is None or self._anchor.device != input_img.device:
                self._anchor = torch.zeros(1, device=input_img.device, requires_grad=True)
            return _ClassifierFunction.apply(self._anchor, self, input_img, keys)
        return self._engine.forward_classifier(input_img, self.training, keep=False, keys=keys)[0]


def get_wide_resnet(name, drop_rate, input_channels=1, num_classes=10, small_input=False, data_parallel=True, compute_dtype="bf16"):
    """classifier_model/wideresnet.py:128-141: name = 'wideresnet-D-W'"""
    depth, width = re.findall(r'\d+', name)           # ValueError if not exactly two integers
    return WideResNetClassifier(depth=int(depth), width=int(width), drop_rate=drop_rate, num_input_channels=input_channels,
                                data_parallel=data_parallel, small_input=small_input, num_classes=num_classes,
                                compute_dtype=compute_dtype)


class _CEFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, label):
        B, K = logits.shape
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        L.call("sv_ce_fwd", _p(logits), _p(label), B, K, None, _p(loss), _st())
        ctx.save_for_backward(logits, label)
        return loss

    @staticmethod
    def backward(ctx, gout):
        logits, label = ctx.saved_tensors
        B, K = logits.shape
        gout = gout.contiguous().float()
        d = torch.empty_like(logits)
        L.call("sv_ce_bwd", _p(logits), _p(label), B, K, _p(gout), _p(d), _st())
        return d, None


class CrossEntropyLoss(nn.Module):
    """nn.CrossEntropyLoss() as main_classifier.py:101 builds it: mean over the batch of logsumexp(logits) - logits[label], on
    fp32 logits [B, K] and int64 labels [B].  Only the default constructor arguments are implemented.  A label outside [0, K)
    gives a NaN loss (and a zero gradient row) instead of torch's device-side assertion."""

    def __init__(self, weight=None, size_average=None, ignore_index=-100, reduce=None, reduction="mean", label_smoothing=0.0):
        super(CrossEntropyLoss, self).__init__()
        if (weight is not None or size_average is not None or ignore_index != -100 or reduce is not None or reduction != "mean"
                or label_smoothing != 0.0):
            raise NotImplementedError("CrossEntropyLoss: only the defaults (mean reduction, no class weights, no label smoothing, "
                                      "ignore_index=-100 unused) are implemented -- what main_classifier.py:101 constructs")

    def forward(self, logits, label):
        if not logits.is_cuda or not label.is_cuda:
            raise L.ShotVaeHipError("CrossEntropyLoss: inputs must be on an MI355X (no CPU fallback)")
        if logits.dim() != 2 or label.dim() != 1 or label.shape[0] != logits.shape[0] or logits.shape[0] == 0:
            raise ValueError("CrossEntropyLoss: logits [B, K] and labels [B] with B > 0; got %s and %s"
                             % (tuple(logits.shape), tuple(label.shape)))
        if logits.dtype != torch.float32 or label.dtype != torch.int64:
            raise TypeError("CrossEntropyLoss: fp32 logits and int64 labels; got %s and %s" % (logits.dtype, label.dtype))
        return _CEFunction.apply(logits.contiguous(), label.contiguous())


def classifier_train_step(model, criterion, optimizer, image, label, distributed=False, return_outputs=False):
    """The body of the loop at main_classifier.py:191-198: forward, loss, backward, (all-reduce,) optimizer step, zero_grad.
    image / label: device tensors.  optimizer=None: gradients only.  Returns the loss (a device scalar: the reference's
    loss.item() is left to the caller); with return_outputs (loss, logits)."""
    if distributed == "bucketed":
        raise ValueError("classifier_train_step: distributed='bucketed' is the SHOT-VAE's decoder-first exchange; the classifier "
                         "has no decoder bucket (use distributed=True: one all-reduce of the flat gradient buffer)")
    model.last_dropout_keys = []
    logits = model(image.float())
    loss = criterion(logits, label.long())
    loss.backward()
    if optimizer is not None:
        apply_update(model, optimizer, distributed)
    return (loss.detach(), logits.detach()) if return_outputs else loss.detach()


class GraphedClassifierStep(GraphedStep):
    """classifier_train_step's forward, loss and backward captured once into a hipGraph and replayed; the gradient exchange and
    the optimizer step stay outside, as in GraphedTrainStep.  The `warmup` eager steps of the constructor are real training steps
    on the construction batch.  With drop_rate > 0 the model needs rng='device' (the keys are then drawn by every replay)."""

    def __init__(self, model, criterion, optimizer, image, label, distributed=False, warmup=2):
        if distributed == "bucketed":
            raise ValueError("GraphedClassifierStep: the classifier has no decoder bucket (distributed=True or False)")
        assert model.drop_rate == 0 or model.rng == "device", \
            "graph capture with dropout needs device-side keys: WideResNetClassifier(..., rng='device')"
        self.model, self.opt, self.distributed = model, optimizer, distributed
        self.criterion = criterion
        self.image, self.label = image.float().clone(), label.long().clone()
        self._warm_up(warmup)
        self._capture()

    def _body(self):
        return classifier_train_step(self.model, self.criterion, None, self.image, self.label)

    def __call__(self, image=None, label=None):
        if image is not None:
            self.image.copy_(image)
            self.label.copy_(label)
        self.graph.replay()
        self._update()
        return self.losses


class ClassifierEvaluator:
    """Running results of one loop of test() (main_classifier.py:219-237 / :247-272): the batch losses averaged with the batch
    sizes as weights (lib/utils/avgmeter.py), top-1 and top-k accuracy over all samples.  Everything stays on the device;
    result() does the one device-to-host copy.  Top-k is counted on the logits (softmax is monotone)."""

    def __init__(self, model, topk=5):
        self.model, self.topk = model, topk
        self.reset()

    def reset(self):
        self.acc = None          # device: [sum loss * B, top1 hits, topk hits]
        self.count = 0

    def update(self, image, label):
        model = self.model
        if not image.is_cuda:
            raise L.ShotVaeHipError("ClassifierEvaluator: inputs must be on an MI355X (no CPU fallback)")
        image = image.float().contiguous()
        label = label.long().contiguous()
        B = image.size(0)
        was_training = model.training
        model.eval()                                                     # :214
        try:
            with torch.no_grad():
                logits = model(image)                                    # :222-223
                K = logits.shape[1]
                loss = torch.empty((), dtype=torch.float32, device=image.device)
                L.call("sv_ce_fwd", _p(logits), _p(label), B, K, None, _p(loss), _st())          # :225
                if self.acc is None:
                    self.acc = torch.zeros(3, dtype=torch.float32, device=image.device)
                self.acc[0] += B * loss                                                          # :226
                L.call("sv_topk_hits", _p(logits), _p(label), B, K, self.topk, _p(self.acc[1:]), _st())      # :234-237
        finally:
            model.train(was_training)
        self.count += B
        return logits, loss

    def result(self):
        """dict(loss, top1, top5) as Python floats (one host sync)"""
        if self.acc is None or self.count == 0:
            return dict(loss=0.0, top1=0.0, top5=0.0)
        a = (self.acc / self.count).tolist()
        return dict(loss=a[0], top1=a[1], top5=a[2])


def evaluate_classifier(model, batches, topk=5):
    """One loop of test(): `batches` yields (image, label) device tensors; returns dict(loss, top1, top5).  The reference returns
    the test set's top-1 (:277)."""
    ev = ClassifierEvaluator(model, topk)
    for image, label in batches:
        ev.update(image, label)
    return ev.result()
