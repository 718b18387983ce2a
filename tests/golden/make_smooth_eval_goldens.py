"""Generate the smooth-ELBO inference golden vectors by running the REFERENCE models on the CPU (sibling of make_goldens.py's
run_smooth_case, whose ``.cuda()`` no-op shim and import path it follows): smooth_vae_model/svhn_vae.py (svhn_VAE) and
mnist_vae.py (mnist_VAE) in eval mode, driven the way Trainer.eval (main_smooth_ELBO_svhn.py:217-226) and a user of a trained
model drive them.

The state is oracle.smooth_oracle.make_state(kind) with ``fc_alphas.0.weight`` multiplied by HEAD_SCALE = 400: under the closed-form
initialisation alone alpha is uniform to 1e-3 (median top-2 margin 7e-4) and every argmax would be a coin toss under bf16; with the
scaled head the logits have a standard deviation of about 4.7 and the predictions cover most classes.

Recorded per kind, for the 256 closed-form images of eval_images(kind): the float32 logits, alpha = model.encode(x)['disc'][0],
pred = torch.max(alpha, 1)[1], the labels of eval_labels(pred) (every third one wrong) and the hit count of the reference's own
comparison np.sum(pred == label); for the first N_REC = 8 images model(x)[0], model(x, foreign label)[0] and
model.decode(latent) of one explicit latent matrix.  The fixtures hold labels and OUTPUTS only: the functions below regenerate the
inputs wherever a test needs them.

    python tests/golden/make_smooth_eval_goldens.py

Writes tests/golden/ref_smooth_eval_svhn.npz and ref_smooth_eval_mnist.npz.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import torch                                  # noqa: E402
from oracle import closed_form as C           # noqa: E402
from oracle import smooth_oracle as SO        # noqa: E402

KINDS = ("svhn", "mnist")
HEAD_SCALE = 400.0
N_REC, CONT, DISC = 8, 32, 10


def eval_state(kind):
    """the closed-form state with the class head scaled (see above)"""
    st = SO.make_state(kind, CONT, DISC)
    st["fc_alphas.0.weight"] = st["fc_alphas.0.weight"] * HEAD_SCALE
    return st


def eval_images(kind):
    """256 closed-form images in [-1, 1]: the 200 + 56 of oracle.smooth_oracle.make_inputs"""
    return torch.cat(SO.make_inputs(kind, 200, 56)[:2])


def eval_labels(pred):
    """labels that make two of three predictions right: pred for i % 3 != 0, else (pred + 1) % 10"""
    i = torch.arange(pred.shape[0])
    return torch.where(i % 3 != 0, pred, (pred + 1) % DISC)


def recon_inputs():
    """for the first N_REC images: the foreign labels of the class swap, and the explicit latent matrix [N_REC, CONT + DISC] =
    [closed-form normal z | one-hot class]"""
    foreign = (torch.arange(N_REC) * 3 + 1) % DISC
    cls = (torch.arange(N_REC) * 7 + 3) % DISC
    latent = torch.cat([C.normal((N_REC, CONT), 9700), torch.nn.functional.one_hot(cls, DISC).float()], dim=1)
    return foreign, latent


def run_case(kind):
    import numpy as np
    import torch.nn as nn
    sys.path.insert(0, HERE)
    import make_goldens as MG
    torch.Tensor.cuda = lambda self, *a, **k: self
    nn.Module.cuda = lambda self, *a, **k: self
    sys.path.insert(0, MG.REF)
    if kind == "svhn":
        from smooth_vae_model.svhn_vae import svhn_VAE as Model
    else:
        from smooth_vae_model.mnist_vae import mnist_VAE as Model
    model = Model(img_size=(SO.KINDS[kind]["in_ch"], 32, 32), latent_spec={"cont": CONT, "disc": [DISC]}, temperature=0.67,
                  use_cuda=False)
    model.load_state_dict(eval_state(kind))
    model.eval()
    x = eval_images(kind)
    foreign, latent = recon_inputs()
    with torch.no_grad():
        hidden = model.features_to_hidden(model.img_to_features(x).view(x.shape[0], -1))
        logits = model.fc_alphas[0](hidden)
        alpha = model.encode(x)["disc"][0]
        pred = torch.max(alpha, 1)[1]
        label = eval_labels(pred)
        hits = np.sum(pred.cpu().numpy() == label.cpu().numpy())               # Trainer.eval's comparison (:223-225)
        rec = model(x[:N_REC])[0]
        rec_label = model(x[:N_REC], foreign)[0]
        rec_latent = model.decode(latent)
    path = os.path.join(HERE, "ref_smooth_eval_%s.npz" % kind)
    np.savez_compressed(path, logits=logits.numpy(), alpha=alpha.numpy(), pred=pred.numpy(), label=label.numpy(), hits=np.array(hits),
                        rec=rec.numpy(), rec_label=rec_label.numpy(), rec_latent=rec_latent.numpy())
    top2 = torch.topk(logits, 2, dim=1).values
    print(kind, "logit std %.2f" % float(logits.std()), "classes predicted", len(set(pred.tolist())), "hits", int(hits),
          "median top-2 gap %.3f" % float((top2[:, 0] - top2[:, 1]).median()), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    sys.path.insert(0, HERE)
    import make_goldens as MG
    assert os.path.isdir(MG.REF), "reference not mounted; goldens are generated in the build container"
    torch.set_num_threads(8)
    for kind in KINDS:
        run_case(kind)
