"""The latent space as a picture: the t-SNE map of the posteriors of a set of images (shot_vae_amd.evaluate_embedding), one dot per
image coloured by its label, written as binary PPM in the style of tools/generate_grid.py / tools/neighbor_grid.py.
--model shot: a VariationalAutoEncoder (--encoder, --classes, --latent); --model smooth: an svhn_VAE / mnist_VAE (--channels 3 / 1).
--state FILE: a state dict saved with torch.save; without it the default initialisation.
--images FILE.npy: uint8 [N, 32, 32, ch]; --labels FILE.npy: integers [N]; without them uniform noise images with labels i mod classes
(a smoke run of the tool).
Needs an MI355X.
Usage: python tools/embedding_plot.py [--model shot] [--encoder wideresnet-28-2] [--state FILE] [--images X.npy --labels Y.npy]
                                      [--metric kl] [--perplexity 30] [--iters 1000] [--size 768] [--dot 3] [--batch 512] [--dtype bf16]
                                      [--out embedding.ppm]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shot_vae_amd as S                                   # noqa: E402
from tools.generate_grid import write_pnm                  # noqa: E402
from tools.neighbor_grid import to_input                   # noqa: E402

# ten colours told apart on white (the "tab10" hues), repeated beyond ten classes
PALETTE = np.array([(31, 119, 180), (255, 127, 14), (44, 160, 44), (214, 39, 40), (148, 103, 189), (140, 86, 75), (227, 119, 194),
                    (127, 127, 127), (188, 189, 34), (23, 190, 207)], dtype=np.uint8)


def scatter(y, labels, size=768, dot=3, margin=8):
    """y float [N, 2], labels int [N] (a negative label is drawn black) -> uint8 [size, size, 3]: the points scaled by ONE factor into the
    square (the map's distances keep their proportions), later rows drawn over earlier ones"""
    y = np.asarray(y, dtype=np.float64)
    lo, hi = y.min(axis=0), y.max(axis=0)
    span = max(float((hi - lo).max()), 1e-30)
    pix = np.rint(margin + (y - 0.5 * (lo + hi)) / span * (size - 2 * margin - dot) + 0.5 * (size - 2 * margin - dot)).astype(np.int64)
    img = np.full((size, size, 3), 255, dtype=np.uint8)
    for (cx, cy), lab in zip(pix, np.asarray(labels)):
        img[size - dot - cy:size - cy, cx:cx + dot] = PALETTE[lab % len(PALETTE)] if lab >= 0 else 0          # (y grows upwards)
    return img


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="shot", choices=("shot", "smooth"))
    ap.add_argument("--encoder", default="wideresnet-28-2")
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--latent", type=int, default=None)
    ap.add_argument("--state")
    ap.add_argument("--images")
    ap.add_argument("--labels")
    ap.add_argument("--metric", default="kl")
    ap.add_argument("--perplexity", type=float, default=30.0)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--size", type=int, default=768)
    ap.add_argument("--dot", type=int, default=3)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp32"))
    ap.add_argument("--out", default="embedding.ppm")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/embedding_plot.py runs the model on an MI355X: no GPU here"
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
    if a.images:
        images = np.load(a.images)
        assert images.dtype == np.uint8 and images.ndim == 4 and images.shape[1:] == (32, 32, a.channels), "%s: uint8 [N, 32, 32, ch]" % a.images
        labels = np.load(a.labels).astype(np.int64).reshape(-1) if a.labels else np.full(len(images), -1, dtype=np.int64)
        assert len(labels) == len(images), "%d labels for %d images" % (len(labels), len(images))
    else:
        images = np.random.default_rng(0).integers(0, 256, size=(512, 32, 32, a.channels), dtype=np.uint8)
        labels = np.arange(len(images), dtype=np.int64) % a.classes
    data = [(to_input(images[i:i + a.batch], smooth), torch.from_numpy(labels[i:i + a.batch]).cuda()) for i in range(0, len(images), a.batch)]
    res = S.evaluate_embedding(m, data, chunk_rows=a.batch, metric=a.metric, perplexity=a.perplexity, n_iter=a.iters)
    write_pnm(a.out, scatter(res["embedding"].cpu().numpy(), labels, a.size, a.dot))
    print("wrote %s (%d points under %s, perplexity %g, %d iterations): KL %.4f, neighbourhood hit %.4f, preservation %.4f"
          % (a.out, len(images), a.metric, a.perplexity, res["n_iter"], res["kl"], res["neighbourhood_hit"], res["neighbourhood_preservation"]))


if __name__ == "__main__":
    main()
