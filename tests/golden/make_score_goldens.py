"""Generate the per-image score fixture by running the REFERENCE implementation on CPU (sibling of make_infer_goldens.py, whose
pattern it follows: make_goldens.py's ``.cuda()`` no-op shim and reference import, the closed-form state of oracle/closed_form.py).

The reference model in eval mode on wideresnet-10-1, K = 10, B = 4 closed-form images: its three inference heads, and its own
``VAECriterion`` (lib/criterion.py:32-57) applied to batches of ONE -- which is what a per-image score is.  Recorded:
  mu, ls, la                 the heads' outputs
  kl_c [B], kl_d [B]         the criterion's two KL terms of image b alone
  nll_mu_bce / nll_mu_mse    [B, K]: the criterion's reconstruction term of image b against the reference decoder's output for
                             [mu_b | onehot k], BCE mode and MSE mode with x_sigma = X_SIGMA
  z [B, S, ldc]              the sweep stream's z = mu + exp(ls) * n(ROW0 + b, s, .) for KEY, from the float64 numpy restatement of
                             tests/_score_ref.py, rounded once to fp32 (an INPUT of the next two, kept so that they stay usable
                             if the stream's definition ever changes)
  nll_s_bce / nll_s_mse      [B, S, K]: the same reconstruction terms at [z_{b,s} | onehot k]
The fixture holds the reference's OUTPUTS only (and z); score_inputs() below regenerates the images wherever a test needs them.

    python tests/golden/make_score_goldens.py

Writes tests/golden/ref_score_wrn10_1.npz.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import torch                                  # noqa: E402
from oracle import closed_form as C           # noqa: E402

TAG, NAME = "ref_score_wrn10_1", "wideresnet-10-1"
K, B, LDC, S = 10, 4, 128, 3
X_SIGMA = 0.5
KEY, ROW0 = 0x5C0DE5EED1234, 3
IMAGE_STREAM = 9700


def score_inputs():
    """the closed-form images of the fixture, [B, 3, 32, 32] in [0, 1)"""
    return C.uniform((B, 3, 32, 32), IMAGE_STREAM)


def run_score_case():
    import numpy as np
    sys.path.insert(0, HERE)
    import make_goldens as MG
    from tests._score_ref import sweep_z
    VAE, VAECriterion, *_ = MG.import_reference()
    model = VAE(encoder_name=NAME, num_input_channels=3, drop_rate=0, img_size=(32, 32), data_parallel=False,
                continuous_latent_dim=LDC, disc_latent_dim=K, sample_temperature=0.67, small_input=True)
    model.load_state_dict(C.make_state(NAME, K=K))
    model.eval()
    crit = {"bce": VAECriterion(discrete_dim=K, x_sigma=1, bce_reconstruction=True),
            "mse": VAECriterion(discrete_dim=K, x_sigma=X_SIGMA, bce_reconstruction=False)}
    x = score_inputs()
    eye = torch.eye(K)
    with torch.no_grad():
        feat = model.global_avg(model.feature_extractor(x)).view(B, -1)
        mu = model.continuous_inference.mean(feat)
        ls = model.continuous_inference.log_sigma(feat)
        la = model.disc_latent_inference(feat)
        z = torch.from_numpy(sweep_z(KEY, ROW0, B, S, LDC, mu.numpy(), ls.numpy()).astype(np.float32))      # [B, S, ldc]
        out = dict(mu=mu.numpy(), ls=ls.numpy(), la=la.numpy(), z=z.numpy(), kl_c=np.zeros(B, np.float32), kl_d=np.zeros(B, np.float32))
        for m in crit:
            out["nll_mu_" + m] = np.zeros((B, K), np.float32)
            out["nll_s_" + m] = np.zeros((B, S, K), np.float32)
        for b in range(B):
            one = slice(b, b + 1)
            for k in range(K):
                for s in range(-1, S):                   # -1: z = mu
                    zb = mu[one] if s < 0 else z[one, s]
                    rec = model.feature_reconstructor(torch.cat([zb, eye[k:k + 1]], dim=1)[:, :, None, None])
                    for m, c in crit.items():
                        r, klc, kld = c(x[one], rec, mu[one], ls[one], la[one])
                        if s < 0:
                            out["nll_mu_" + m][b, k] = float(r)
                        else:
                            out["nll_s_" + m][b, s, k] = float(r)
                        out["kl_c"][b], out["kl_d"][b] = float(klc), float(kld)
    path = os.path.join(HERE, TAG + ".npz")
    np.savez_compressed(path, **out)
    print(TAG, {k: (v.shape, float(np.abs(v).mean())) for k, v in out.items()}, "bytes", os.path.getsize(path))


if __name__ == "__main__":
    sys.path.insert(0, HERE)
    import make_goldens as MG
    assert os.path.isdir(MG.REF), "reference not mounted; goldens are generated in the build container"
    torch.set_num_threads(8)
    run_score_case()
