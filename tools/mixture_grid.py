"""Samples from a mixture fitted to a SHOT-VAE's codes beside samples from the prior, written as binary PPM (PGM for one channel) with
numpy alone ("ex-post density estimation" to look at):
  OUT_mixture.ppm   K rows x n columns: row k = n images of class k decoded from codes drawn from the fitted GaussianMixture
                    (generate_from_mixture)
  OUT_prior.ppm     the same grid with z ~ N(0, tau^2 I) (VariationalAutoEncoder.generate), the same key
--state FILE: the model's state dict saved with torch.save; without it the default initialisation.
--images FILE.npy: uint8 [N, 32, 32, ch] images whose posterior means the mixture is fitted to; --mixture FILE: a GaussianMixture
state_dict saved with torch.save instead (then no images are needed); --save-mixture FILE writes the fitted one.
Needs an MI355X.
Usage: python tools/mixture_grid.py --encoder wideresnet-28-2 --classes 10 [--state FILE] (--images FILE.npy | --mixture FILE)
                                    [--components 10] [--n 8] [--tau 1.0] [--key 0] [--dtype bf16] [--out grid]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shot_vae_amd as S                                   # noqa: E402
from tools.generate_grid import tile, to_u8, write_pnm     # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--encoder", default="wideresnet-28-2")
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--latent", type=int, default=128)
    ap.add_argument("--state")
    ap.add_argument("--images")
    ap.add_argument("--mixture")
    ap.add_argument("--save-mixture")
    ap.add_argument("--components", type=int, default=10)
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--tau", type=float, default=1.0)
    ap.add_argument("--key", type=int, default=0)
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp32"))
    ap.add_argument("--out", default="grid")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/mixture_grid.py runs the model on an MI355X: no GPU here"
    assert bool(a.images) != bool(a.mixture), "one of --images (fit a mixture) and --mixture (load one)"
    K, n = a.classes, a.n
    m = S.VariationalAutoEncoder(a.encoder, num_input_channels=a.channels, img_size=(32, 32), data_parallel=False,
                                 continuous_latent_dim=a.latent, disc_latent_dim=K, small_input=True, compute_dtype=a.dtype)
    if a.state:
        m.load_state_dict(torch.load(a.state, map_location="cpu"))
    m = m.cuda().eval()
    if a.mixture:
        state = torch.load(a.mixture, map_location="cpu")
        gm = S.GaussianMixture(int(state["k"]), int(state["dim"])).load_state_dict(state, device="cuda")
    else:
        src = np.load(a.images)
        assert src.dtype == np.uint8 and src.ndim == 4 and src.shape[1:] == (32, 32, a.channels), "--images: uint8 [N, 32, 32, ch]"
        x = torch.from_numpy(src).cuda().permute(0, 3, 1, 2).float().div(255.0).contiguous()
        res = S.evaluate_mixture(m, [x[i:i + 256] for i in range(0, len(x), 256)], k=a.components)
        gm = res["mixture"]
        print("fitted %d components to %d codes: mean log-likelihood %.4f (prior %.4f), BIC %.1f, %s after %d iterations"
              % (gm.k, res["n_fit"], res["ll_fit"], res["prior_ll_fit"], res["bic"], "converged" if gm.converged_ else "NOT converged",
                 gm.n_iter_))
    if a.save_mixture:
        torch.save({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in gm.state_dict().items()}, a.save_mixture)
    labels = torch.arange(K, device="cuda").repeat_interleave(n)            # row k = class k
    write_pnm(a.out + "_mixture.ppm", tile(to_u8(S.generate_from_mixture(m, gm, labels, a.key)), K, n))
    write_pnm(a.out + "_prior.ppm", tile(m.generate(labels, a.key, tau=a.tau, dtype="uint8").cpu().numpy(), K, n))
    print("wrote %s_mixture.ppm and %s_prior.ppm (%d x %d each)" % (a.out, a.out, K, n))


if __name__ == "__main__":
    main()
