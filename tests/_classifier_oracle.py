"""CPU oracle of the classifier-only WideResNet baseline  --  TEST INFRASTRUCTURE ONLY (imported by the classifier tests, never by
the product).

A functional torch-CPU restatement of classifier_model/wideresnet.py:68-125 (forward), nn.CrossEntropyLoss() (main_classifier.py:
101) and the step of main_classifier.py:191-198 over a flat ``state`` dict with the reference's state_dict names
(data_parallel=False).  The encoder is the SHOT-VAE's under other names, so the units, the BatchNorm and the SGD step are those of
oracle/shotvae_oracle.py, reached through a renamed view of the state (the tensors are shared: running statistics update in place).
``patched()`` makes oracle.closed_form.make_state generate the closed-form state over this key table.

Pinned against the reference by tests/golden/make_classifier_goldens.py -> tests/test_classifier_cpu.py.
"""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import closed_form as C
from oracle import shotvae_oracle as O

VAE_ENC = "feature_extractor.encoder."
VAE_BN_T = VAE_ENC + "transition.norm."
ENC = "encoder."
BN_T = "global_avg.norm."
FC = "classification.fc."

# tag -> (net, K, B, steps, image stream): the step fixtures of tests/golden/make_classifier_goldens.py.  The stream of the
# wideresnet-28-10 case is chosen: with 2 images and ~5 M LeakyReLU inputs, in most streams the reference's fp32 run puts a few
# pre-activations on the other side of 0 than float64 does, which moves single gradient entries by 1e-4 ... 9e-4 of the largest
# (22 of 26 streams tried); the maker's fp64 check (1e-5) passes for 8800, 8900, 9500 and 9900.
STEP_CASES = {"ref_cls_step_wrn10_1": ("wideresnet-10-1", 10, 8, 2, 7000),
              "ref_cls_step_wrn28_2": ("wideresnet-28-2", 10, 4, 1, 7000),
              "ref_cls_step_wrn28_10_k100": ("wideresnet-28-10", 100, 2, 1, 8800)}
EVAL_CASE = ("ref_cls_eval_wrn10_1", "wideresnet-10-1", 10, 8)
KEY_CASES = (("wideresnet-10-1", 10), ("wideresnet-28-2", 10), ("wideresnet-28-10", 100))
SGD = dict(lr=0.1, momentum=0.9, weight_decay=5e-4)


def _to_vae_key(k):
    """the SHOT-VAE oracle's name of an encoder entry (None for the fc)"""
    if k.startswith(ENC):
        return VAE_ENC + k[len(ENC):]
    if k.startswith(BN_T):
        return VAE_BN_T + k[len(BN_T):]
    return None


def state_shapes(name, in_ch=3, ldc=128, K=10, img=32):
    """Ordered {key: shape} of the reference classifier's state_dict (data_parallel=False): the SHOT-VAE oracle's encoder table
    under the classifier's names, then the fc (ldc is unused: the signature is oracle.shotvae_oracle.state_shapes')."""
    sh = {}
    for k, shape in _orig_state_shapes(name, in_ch, ldc, K, img).items():
        if k.startswith(VAE_BN_T):
            sh[BN_T + k[len(VAE_BN_T):]] = shape
        elif k.startswith(VAE_ENC):
            sh[ENC + k[len(VAE_ENC):]] = shape
    cfeat = sh[BN_T + "weight"][0]
    sh[FC + "weight"] = (K, cfeat)
    sh[FC + "bias"] = (K,)
    return sh


_orig_state_shapes = O.state_shapes


@contextlib.contextmanager
def patched():
    """While active, oracle.shotvae_oracle.state_shapes (and with it oracle.closed_form.make_state) is the classifier's key table."""
    saved = O.state_shapes
    O.state_shapes = state_shapes
    try:
        yield
    finally:
        O.state_shapes = saved


def make_state(name, K=10, dt=torch.float32, requires_grad=False):
    with patched():
        st = C.make_state(name, K=K)
    for k in st:
        if st[k].dtype.is_floating_point:
            st[k] = st[k].to(dt)
        if requires_grad and O.is_param(k):
            st[k].requires_grad_(True)
    return st


def forward(st, name, x, training=True, update=True):
    """classifier_model/wideresnet.py:120-125: encoder, BatchNorm + LeakyReLU + average pool, Linear -> raw logits"""
    view = {_to_vae_key(k): v for k, v in st.items() if _to_vae_key(k) is not None}
    feat = O.encoder_forward(view, name, x, training, update)
    return F.linear(feat.mean((2, 3)), st[FC + "weight"], st[FC + "bias"])


def cross_entropy(logits, label):
    """nn.CrossEntropyLoss(): mean_b (logsumexp(z_b) - z_b[label_b])"""
    return (torch.logsumexp(logits, 1) - logits.gather(1, label.view(-1, 1)).squeeze(1)).mean()


def make_batch(B, K, step=0, dt=torch.float32, stream0=7000):
    """the closed-form batch of step `step`: images U[0, 1) from hash stream stream0 + 10 * step, labels that cover 0 and spread
    over the classes"""
    image = C.uniform((B, 3, 32, 32), stream0 + 10 * step).to(dt)
    label = (torch.arange(B) * 7 + 3 * step) % K
    return image, label


def sample_idx(n, k=16):
    return np.unique(np.linspace(0, n - 1, num=min(k, n)).astype(np.int64))


def run_steps(name, K, B, steps, stream0=7000, dt=torch.float32, hook=None):
    """`steps` consecutive steps (forward, CE, backward, SGD) from the closed-form state in dtype dt.  Returns (per-step dicts:
    logits, loss, grad_norm, grad_sample, grads), the final state, the parameter keys.  hook(step): called before each forward."""
    st = make_state(name, K, dt, requires_grad=True)
    pk = [k for k in st if O.is_param(k)]
    mom, outs = {}, []
    for s in range(steps):
        if hook is not None:
            hook(s)
        image, label = make_batch(B, K, s, dt, stream0)
        logits = forward(st, name, image, training=True)
        loss = cross_entropy(logits, label)
        loss.backward()
        out = dict(logits=logits.detach(), loss=loss.detach())
        out["grad_norm"] = np.array([float(st[k].grad.double().norm()) for k in pk])
        out["grad_sample"] = np.concatenate([st[k].grad.reshape(-1)[torch.from_numpy(sample_idx(st[k].numel()))].double().numpy()
                                             for k in pk])
        out["grads"] = {k: st[k].grad.detach().clone() for k in pk}
        outs.append(out)
        O.sgd_step(st, mom, **SGD)
    return outs, st, pk


def run_eval(name, K, B, dt=torch.float32):
    """eval-mode forward with the closed-form running statistics: logits, CE, top-1 and top-5 hit counts"""
    st = make_state(name, K, dt)
    image, label = make_batch(B, K, 0, dt)
    with torch.no_grad():
        logits = forward(st, name, image, training=False)
        loss = cross_entropy(logits, label)
    top = torch.topk(logits, 5, dim=1).indices
    return dict(logits=logits, loss=loss, top1=int((top[:, :1] == label.view(-1, 1)).sum()), top5=int((top == label.view(-1, 1)).sum()))
