"""What tests/test_smooth_infer_cpu.py and tests/test_smooth_infer_gpu.py share: the fixtures of
tests/golden/make_smooth_eval_goldens.py with their regenerated inputs, the fp32 CPU oracle on them, and two restatements of the same
forward (oracle/smooth_oracle.py: forward) that the GPU tests' allowances are MEASURED from -- never from a GPU result:

  * float64: the error of the fp32 oracle against it, times 8, is what an fp32-mode GPU output may be off the fixture by (the
    project's rule, tests/test_head_loss_kernels_gpu.py: max |a - ref| / max |ref| over the tensor, at least 8 x 2^-24);
  * bf16 emulation of the ENCODER -- weights, input and every layer's output rounded to bf16, fp32 accumulation, fp32 biases, which
    is what the bf16 path stores -- its largest logit difference from the fp32 oracle, times 4, is the top-2 gap below which a
    row's argmax is "undecided": predictions are compared on the decided rows only, in bf16 and fp32 mode alike.

Everything is computed once per kind (lru_cache) and must be left unchanged by its users."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import smooth_oracle as SO
from tests import _cases as T
from tests.golden import make_smooth_eval_goldens as G

HALF_ULP = 2.0 ** -24
MAX_UNDECIDED = 64                    # 25 % of the 256 images


def restated(st, kind, x, label=None, dtype=torch.float64, bf16=False):
    """oracle.smooth_oracle.forward(training=False) in `dtype`; bf16=True: weights, input and every layer's output rounded to bf16
    (biases and accumulation stay in `dtype`).  -> dict(mean, logvar, logits, alpha, rec)"""
    r = (lambda t: t.to(torch.bfloat16).to(dtype)) if bf16 else (lambda t: t)
    w = lambda k: r(st[k].to(dtype))
    b = lambda k: st[k].to(dtype)
    h = r(x.to(dtype))
    for i in (0, 2, 4):
        h = F.relu(r(F.conv2d(h, w("img_to_features.%d.weight" % i), b("img_to_features.%d.bias" % i), 2, 1)))
    hid = F.relu(r(F.linear(h.reshape(x.shape[0], -1), w("features_to_hidden.0.weight"), b("features_to_hidden.0.bias"))))
    mean = r(F.linear(hid, w("fc_mean.weight"), b("fc_mean.bias")))
    logvar = r(F.linear(hid, w("fc_log_var.weight"), b("fc_log_var.bias")))
    logits = r(F.linear(hid, w("fc_alphas.0.weight"), b("fc_alphas.0.bias")))
    alpha = F.softmax(logits, dim=1)
    c = F.one_hot(alpha.argmax(1) if label is None else label, alpha.shape[1]).to(dtype)
    rec = decode_restated(st, kind, torch.cat([mean, c], 1), dtype, bf16)
    return dict(mean=mean, logvar=logvar, logits=logits, alpha=alpha, rec=rec)


def decode_restated(st, kind, lat, dtype=torch.float64, bf16=False):
    """the decoder of oracle.smooth_oracle.forward (svhn_vae.py:270-281) in `dtype`"""
    r = (lambda t: t.to(torch.bfloat16).to(dtype)) if bf16 else (lambda t: t)
    w = lambda k: r(st[k].to(dtype))
    b = lambda k: st[k].to(dtype)
    f = F.relu(r(F.linear(r(lat.to(dtype)), w("latent_to_features.0.weight"), b("latent_to_features.0.bias"))))
    f = F.relu(r(F.linear(f, w("latent_to_features.2.weight"), b("latent_to_features.2.bias"))))
    f = f.view(-1, SO.KINDS[kind]["widths"][2], 4, 4)
    f = F.relu(r(F.conv_transpose2d(f, w("features_to_img.0.weight"), b("features_to_img.0.bias"), 2, 1)))
    f = F.relu(r(F.conv_transpose2d(f, w("features_to_img.2.weight"), b("features_to_img.2.bias"), 2, 1)))
    return torch.tanh(r(F.conv_transpose2d(f, w("features_to_img.4.weight"), b("features_to_img.4.bias"), 2, 1)))


def rel(a, ref):
    return T.rel_err(a.detach().cpu().numpy() if torch.is_tensor(a) else a, ref.detach().cpu().numpy() if torch.is_tensor(ref) else ref)


def allowance(f32, f64):
    """8 x the fp32 restatement's error against float64, at least 8 x 2^-24"""
    return 8.0 * max(rel(f32, f64), HALF_ULP)


@functools.lru_cache(maxsize=None)
def case(kind):
    """Everything about one fixture, computed once:
      g          the fixture (numpy), st the state, x the 256 images, label the fixture's labels, foreign / latent of recon_inputs()
      oracle     fp32 CPU oracle: alpha, pred, rec (first 8, predicted class), rec_label (first 8, foreign label)
      tol_alpha, tol_rec, tol_rec_label, tol_rec_latent     the fp32-mode allowances (8 x rule)
      gap        4 x the largest logit difference between the fp32 oracle and the bf16-emulated encoder
      decided    bool [256]: the top-2 gap of the FIXTURE's logits is at least `gap`"""
    g = {k: v for k, v in T.load("ref_smooth_eval_" + kind).items()}
    st, x = G.eval_state(kind), G.eval_images(kind)
    foreign, latent = G.recon_inputs()
    n = G.N_REC
    with torch.no_grad():
        zero = torch.zeros(x.shape[0], G.CONT)
        rec_all, _, _, alpha, _ = SO.forward(st, kind, x, zero, training=False)
        rec_label = SO.forward(st, kind, x[:n], zero[:n], label=foreign, training=False)[0]
        f32 = restated(st, kind, x, dtype=torch.float32)
        f64 = restated(st, kind, x)
        emu = restated(st, kind, x, dtype=torch.float32, bf16=True)
        f64_label = restated(st, kind, x[:n], label=foreign)
        f32_label = restated(st, kind, x[:n], label=foreign, dtype=torch.float32)
        lat32, lat64 = decode_restated(st, kind, latent, torch.float32), decode_restated(st, kind, latent)
    gap = 4.0 * float((emu["logits"] - f32["logits"]).abs().max())
    top2 = np.sort(g["logits"].astype(np.float64), axis=1)[:, -2:]
    decided = (top2[:, 1] - top2[:, 0]) >= gap
    return dict(g=g, st=st, x=x, label=torch.from_numpy(g["label"]), foreign=foreign, latent=latent,
                oracle=dict(alpha=alpha, pred=alpha.argmax(1), rec=rec_all[:n], rec_label=rec_label, logits=f32["logits"], rec_latent=lat32),
                tol_alpha=allowance(f32["alpha"], f64["alpha"]), tol_rec=allowance(f32["rec"][:n], f64["rec"][:n]),
                tol_rec_label=allowance(f32_label["rec"], f64_label["rec"]), tol_rec_latent=allowance(lat32, lat64),
                gap=gap, decided=decided)
