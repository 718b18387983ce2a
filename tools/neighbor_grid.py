"""Retrieval in latent space as a picture: one row per query image -- the query, then its k nearest gallery images under the
posterior's own geometry (LatentIndex.search over encode_posterior), closest first -- written as binary PPM (PGM for one channel) in
the style of tools/generate_grid.py.
--model shot: a VariationalAutoEncoder (--encoder, --classes, --latent); --model smooth: an svhn_VAE / mnist_VAE (--channels 3 / 1).
--state FILE: a state dict saved with torch.save; without it the default initialisation.
--gallery / --queries FILE.npy: uint8 [N, 32, 32, ch] images; without them uniform noise images (a smoke run of the tool).
--leave-one-out: the queries are the first rows of the gallery; nobody retrieves itself.
Needs an MI355X.
Usage: python tools/neighbor_grid.py [--model shot] [--encoder wideresnet-28-2] [--state FILE] [--gallery G.npy] [--queries Q.npy]
                                     [--k 8] [--metric kl] [--rows 10] [--batch 512] [--dtype bf16] [--out neighbors.ppm]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shot_vae_amd as S                                   # noqa: E402
from tools.generate_grid import tile, write_pnm            # noqa: E402


def neighbor_rows(queries, gallery, idx):
    """uint8 [Q, H, W, ch] queries, uint8 [N, H, W, ch] gallery, int64 [Q, k] indices (-1: an empty slot, drawn white) ->
    uint8 [Q * (k + 1), H, W, ch]: every query followed by its neighbours"""
    Q, k = idx.shape
    out = np.full((Q, k + 1) + queries.shape[1:], 255, dtype=np.uint8)
    out[:, 0] = queries
    for j in range(k):
        ok = idx[:, j] >= 0
        out[ok, j + 1] = gallery[idx[ok, j]]
    return out.reshape((-1,) + queries.shape[1:])


def to_input(u8, smooth):
    x = torch.from_numpy(u8).cuda().permute(0, 3, 1, 2).float().div(255.0)
    return (x * 2.0 - 1.0 if smooth else x).contiguous()                # the smooth models see [-1, 1] (Tanh output)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="shot", choices=("shot", "smooth"))
    ap.add_argument("--encoder", default="wideresnet-28-2")
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--latent", type=int, default=None)
    ap.add_argument("--state")
    ap.add_argument("--gallery")
    ap.add_argument("--queries")
    ap.add_argument("--leave-one-out", action="store_true")
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--metric", default="kl")
    ap.add_argument("--rows", type=int, default=10)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp32"))
    ap.add_argument("--out", default="neighbors.ppm")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/neighbor_grid.py runs the model on an MI355X: no GPU here"
    smooth = a.model == "smooth"
    if smooth:
        m = S.SmoothVAE((a.channels, 32, 32), {"cont": a.latent or 32, "disc": [a.classes]}, compute_dtype=a.dtype)
    else:
        m = S.VariationalAutoEncoder(a.encoder, num_input_channels=a.channels, img_size=(32, 32), data_parallel=False,
                                     continuous_latent_dim=a.latent or 128, disc_latent_dim=a.classes, small_input=True,
                                     compute_dtype=a.dtype)
    if a.state:
        m.load_state_dict(torch.load(a.state, map_location="cpu"))
    m = m.cuda().eval()
    rng = np.random.default_rng(0)

    def images(path, n):
        if not path:
            return rng.integers(0, 256, size=(n, 32, 32, a.channels), dtype=np.uint8)
        src = np.load(path)
        assert src.dtype == np.uint8 and src.ndim == 4 and src.shape[1:] == (32, 32, a.channels), "%s: uint8 [N, 32, 32, ch]" % path
        return src

    gallery = images(a.gallery, 512)
    queries = gallery[:a.rows] if a.leave_one_out else images(a.queries, a.rows)[:a.rows]
    index = None
    for i in range(0, len(gallery), a.batch):
        mu, ls = S.encode_posterior(m, to_input(gallery[i:i + a.batch], smooth))
        if index is None:
            index = S.LatentIndex(mu.shape[1], metric=a.metric)
        index.add(mu, ls)
    mu, ls = S.encode_posterior(m, to_input(queries, smooth))
    dist, idx = index.search(mu, ls, a.k, exclude_self_from=0 if a.leave_one_out else None)
    grid = neighbor_rows(queries, gallery, idx.cpu().numpy())
    write_pnm(a.out, tile(grid, len(queries), a.k + 1))
    print("wrote %s (%d queries x (1 + %d nearest of %d) under %s); nearest value per row: %s"
          % (a.out, len(queries), a.k, len(index), a.metric, ", ".join("%.4g" % v for v in dist[:, 0].tolist())))


if __name__ == "__main__":
    main()
