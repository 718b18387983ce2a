"""CPU oracle of the PreActResNet-18 / 34 encoders  --  TEST INFRASTRUCTURE ONLY (imported by the preact tests, never by the product).

A functional torch-CPU fp32 restatement of shot_vae_model/preactresnet.py:4-133 (basic units) over the flat ``state`` dict
convention of oracle/shotvae_oracle.py (reference state_dict names, data_parallel=False), and ``patched()``: a context manager
that makes the existing oracle's step / eval / M2 functions (and oracle.closed_form.make_state) use this encoder while a test
runs -- oracle/ itself stays as it is and keeps knowing WideResNet only.

Pinned against the reference by tests/golden/make_preact_goldens.py -> tests/test_preact_cpu.py.
"""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import closed_form as C
from oracle import shotvae_oracle as O

STAGE_UNITS = {"preactresnet18": (2, 2, 2, 2), "preactresnet34": (3, 4, 6, 3)}
STAGE_WIDTHS = (64, 128, 256, 512)
STEM = 64
ENC = "feature_extractor.encoder."


def is_preact(name):
    return "preactresnet" in name


def encoder_units(name):
    """[(prefix, cin, cout, stride, has_shortcut)] in network order, and the feature width"""
    units, cin = [], STEM
    for s, (w, n) in enumerate(zip(STAGE_WIDTHS, STAGE_UNITS[name])):
        for u in range(n):
            stride = 2 if (s > 0 and u == 0) else 1
            units.append((ENC + "block%d.preact_block.unit%d" % (s + 1, u + 1), cin, w, stride, stride != 1 or cin != w))
            cin = w
    return units, STAGE_WIDTHS[-1]


def _bn_keys(sh, prefix, c):
    for k, shape in (("weight", (c,)), ("bias", (c,)), ("running_mean", (c,)), ("running_var", (c,)), ("num_batches_tracked", ())):
        sh[prefix + "." + k] = shape


def state_shapes(name, in_ch=3, ldc=128, K=10, img=32):
    """Ordered {key: shape} of the reference state_dict (data_parallel=False); the heads and the decoder are the existing
    oracle's (taken from its own table for a WideResNet, with the feature width replaced)."""
    if not is_preact(name):
        return _orig["state_shapes"](name, in_ch, ldc, K, img)
    units, cfeat = encoder_units(name)
    sh = {ENC + "pre_process.conv0.weight": (STEM, in_ch, 3, 3), ENC + "pre_process.conv0.bias": (STEM,)}
    for p, ci, co, stride, sc in units:
        _bn_keys(sh, p + ".f_block.norm1", ci)
        sh[p + ".f_block.conv1.weight"] = (co, ci, 3, 3)
        _bn_keys(sh, p + ".f_block.norm2", co)
        sh[p + ".f_block.conv2.weight"] = (co, co, 3, 3)
        if sc:
            _bn_keys(sh, p + ".i_block.norm", ci)
            sh[p + ".i_block.conv.weight"] = (co, ci, 1, 1)
    _bn_keys(sh, ENC + "transition.norm", cfeat)
    for k, shape in _orig["state_shapes"]("wideresnet-10-1", in_ch, ldc, K, img).items():
        if k.startswith("feature_extractor."):
            continue
        sh[k] = (shape[0], cfeat) if k.endswith("fc.weight") else shape
    return sh


def encoder_forward(st, name, x, training=True, update=True):
    """preactresnet.py:61-65 (unit), :115-117 (net).  (Dropout: the GPU test multiplies norm2's input by the regenerated masks by
    wrapping O._bn, as tests/test_dropout_gpu.py does for the WideResNet -- every BatchNorm here goes through O._bn.)"""
    if not is_preact(name):
        return _orig["encoder_forward"](st, name, x, training, update)
    units, _ = encoder_units(name)
    t = F.conv2d(x, st[ENC + "pre_process.conv0.weight"], st[ENC + "pre_process.conv0.bias"], stride=1, padding=1)
    for p, ci, co, stride, sc in units:
        c1 = F.conv2d(torch.relu(O._bn(st, p + ".f_block.norm1", t, training, update)), st[p + ".f_block.conv1.weight"], None,
                      stride=stride, padding=1)
        c2 = F.conv2d(torch.relu(O._bn(st, p + ".f_block.norm2", c1, training, update)), st[p + ".f_block.conv2.weight"], None,
                      stride=1, padding=1)
        if sc:          # BatchNorm WITHOUT an activation in front of the 1x1 shortcut (preactresnet.py:54-59)
            t = c2 + F.conv2d(O._bn(st, p + ".i_block.norm", t, training, update), st[p + ".i_block.conv.weight"], None,
                              stride=stride, padding=0)
        else:
            t = c2 + t
    return torch.relu(O._bn(st, ENC + "transition.norm", t, training, update))


_orig = {"state_shapes": O.state_shapes, "encoder_forward": O.encoder_forward}


@contextlib.contextmanager
def patched():
    """While active, oracle.shotvae_oracle.{state_shapes, encoder_forward} (and with them default_init, vae_forward, train_step,
    m2_step and oracle.closed_form.make_state) understand the preactresnet18 / 34 names; WideResNet names are passed through."""
    saved = (O.state_shapes, O.encoder_forward)
    O.state_shapes, O.encoder_forward = state_shapes, encoder_forward
    try:
        yield
    finally:
        O.state_shapes, O.encoder_forward = saved


def _sample_idx(n, k=16):
    return np.unique(np.linspace(0, n - 1, num=min(k, n)).astype(np.int64))


# the ref_step_preact18_br case: (net, K, B_l, B_u)
PREACT_STEP = ("preactresnet18", 10, 8, 8)


def oracle_step(name, K, Bl, Bu, dt=torch.float32):
    """the oracle's run of the ref_step_preact18_br case in dtype dt: outputs, state after one SGD step, parameter keys"""
    with patched():
        st = C.make_state(name, K=K)
        for k in st:
            if st[k].dtype.is_floating_point:
                st[k] = st[k].to(dt)
            if O.is_param(k):
                st[k].requires_grad_(True)
        il, ll, iu, lu = C.make_batch(Bl, Bu, K, stream0=7000)
        nz = C.make_noise(Bl, Bu, K, stream0=9000)
        nz = {k: (v.to(dt) if torch.is_tensor(v) and v.dtype.is_floating_point else v) for k, v in nz.items()}
        out = O.train_step(st, name, il.to(dt), ll, iu.to(dt), nz, O.schedule(10))
    pk = [k for k in st if O.is_param(k)]
    out["grad_norm"] = np.array([float(st[k].grad.double().norm()) for k in pk])
    out["grad_sample"] = np.concatenate([st[k].grad.reshape(-1)[torch.from_numpy(_sample_idx(st[k].numel()))].double().numpy()
                                         for k in pk])
    out["grads"] = {k: st[k].grad.detach().clone() for k in pk}
    O.sgd_step(st, {}, lr=0.1, momentum=0.9, weight_decay=5e-4)
    return out, st, pk
