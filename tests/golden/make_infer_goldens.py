"""Generate the inference golden vectors by running the REFERENCE implementation on CPU (sibling of make_preact_goldens.py, whose
pattern it follows: make_goldens.py's ``.cuda()`` no-op shim and reference import, the closed-form state and batch of
oracle/closed_form.py, under tests/_preact_oracle.patched() so that the PreActResNet key table is known).

The reference model in eval mode, its sub-modules called the way a user of a trained model calls them
(shot_vae_model/vae.py:142-150): ``feature_extractor(x)``, the pooled features, the three inference heads, and
``feature_reconstructor(latent)`` for a closed-form latent [B, ldc + K, 1, 1] = [normal z | one-hot c], and again with a soft class
row.  The fixtures hold the reference's OUTPUTS only; infer_inputs() below regenerates the inputs wherever a test needs them.

    python tests/golden/make_infer_goldens.py

Writes tests/golden/ref_infer_wrn10_1.npz and ref_infer_preact18.npz.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import torch                                  # noqa: E402
from oracle import closed_form as C           # noqa: E402

CASES = {"ref_infer_wrn10_1": "wideresnet-10-1", "ref_infer_preact18": "preactresnet18"}
K, B, LDC = 10, 4, 128


def infer_inputs(B=B, ldc=LDC, K=K):
    """the closed-form inputs of the fixtures: images x [B, 3, 32, 32], z [B, ldc] ~ N(0, 1), labels [B], the soft class rows
    [B, K] (rows of a softmax), and the two latents [B, ldc + K, 1, 1] built from them"""
    _, _, x, label = C.make_batch(B, B, K)
    z = C.normal((B, ldc), 9600)
    soft = torch.softmax(C.normal((B, K), 9601) * 1.5, dim=1)
    onehot = torch.zeros(B, K).scatter_(1, label.view(-1, 1), 1)
    return dict(x=x, z=z, label=label, soft=soft,
                latent_hard=torch.cat([z, onehot], dim=1)[:, :, None, None],
                latent_soft=torch.cat([z, soft], dim=1)[:, :, None, None])


def run_infer_case(tag, name):
    import numpy as np
    sys.path.insert(0, HERE)
    import make_goldens as MG
    VAE, *_ = MG.import_reference()
    model = VAE(encoder_name=name, num_input_channels=3, drop_rate=0, img_size=(32, 32), data_parallel=False,
                continuous_latent_dim=LDC, disc_latent_dim=K, sample_temperature=0.67, small_input=True)
    model.load_state_dict(C.make_state(name, K=K))
    model.eval()
    inp = infer_inputs()
    with torch.no_grad():
        fmap = model.feature_extractor(inp["x"])
        feat = model.global_avg(fmap).view(B, -1)
        mu = model.continuous_inference.mean(feat)
        ls = model.continuous_inference.log_sigma(feat)
        la = model.disc_latent_inference(feat)
        rec_hard = model.feature_reconstructor(inp["latent_hard"])
        rec_soft = model.feature_reconstructor(inp["latent_soft"])
    path = os.path.join(HERE, tag + ".npz")
    np.savez_compressed(path, fmap=fmap.numpy(), feat=feat.numpy(), mu=mu.numpy(), ls=ls.numpy(), la=la.numpy(),
                        rec_hard=rec_hard.numpy(), rec_soft=rec_soft.numpy())
    print(tag, tuple(fmap.shape), float(rec_hard.abs().mean()), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    sys.path.insert(0, HERE)
    import make_goldens as MG
    from tests import _preact_oracle as P
    assert os.path.isdir(MG.REF), "reference not mounted; goldens are generated in the build container"
    torch.set_num_threads(8)
    with P.patched():          # oracle.closed_form.make_state over the PreActResNet key table
        for tag, name in CASES.items():
            run_infer_case(tag, name)
