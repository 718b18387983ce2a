"""Image grids from a smooth-ELBO model (SmoothVAE: svhn_VAE / mnist_VAE), written as binary PPM (svhn; for mnist's one channel PGM, and the
files end in .pgm) with the writer of tools/generate_grid.py:
  OUT_classes.ppm    Dd rows x n columns: row k = n samples of class k (SmoothVAE.generate, z ~ N(0, tau^2 I))
  OUT_traverse.ppm   one block of Dd rows per traversed dimension: row k = class k, the columns sweep that continuous dimension
                     over --steps values in [-range, range] from z = 0 (SmoothVAE.traverse with dim)
  OUT_class_sweep.ppm  Dd x Dd: row k = the first sample of class k re-rendered under every class (SmoothVAE.traverse, dim=None)
--state FILE: a state dict saved with torch.save (the reference's key names); without it the default initialisation.
Needs an MI355X.
Usage: python tools/smooth_grid.py [--kind svhn|mnist] [--state FILE] [--n 8] [--tau 1.0] [--key 0] [--dims 0,1,2] [--steps 9]
                                   [--range 2.5] [--dtype bf16] [--out smooth]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.generate_grid import tile, write_pnm             # noqa: E402


def to_u8(img):
    """images in [-1, 1] (the Tanh range of the trainers' Normalize(0.5, 0.5)), NCHW fp32 -> uint8 NHWC numpy"""
    return ((img.permute(0, 2, 3, 1) + 1.0) * 127.5 + 0.5).floor().clamp(0, 255).to(torch.uint8).cpu().numpy()


def save_grid(path, img, rows, cols):
    """img: [rows * cols, C, H, W] in [-1, 1], row-major -> one PPM / PGM"""
    write_pnm(path, tile(to_u8(img), rows, cols))


def class_samples(model, n, key, tau=1.0):
    """[Dd * n, C, 32, 32]: row k of the grid = n samples of class k, and their z"""
    Dd = model.latent_disc_dim
    labels = torch.arange(Dd, device="cuda").repeat_interleave(n)
    return model.generate(labels, key, tau=tau, return_z=True)


def traversal(model, dims, values):
    """[(len(dims) * Dd) * V, C, 32, 32]: for every dimension of `dims` a block of Dd rows (class k, z = 0 but for that dimension)"""
    Dd, Dc = model.latent_disc_dim, model.latent_cont_dim
    z = torch.zeros(Dd, Dc, device="cuda")
    label = torch.arange(Dd, device="cuda")
    blocks = [model.traverse(z, label, dim=d, values=values) for d in dims]          # each [Dd, V, C, 32, 32]
    return torch.cat(blocks).flatten(0, 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kind", default="svhn", choices=("svhn", "mnist"))
    ap.add_argument("--cont", type=int, default=32)
    ap.add_argument("--disc", type=int, default=10)
    ap.add_argument("--state")
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--tau", type=float, default=1.0)
    ap.add_argument("--key", type=int, default=0)
    ap.add_argument("--dims", default="0,1,2")
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--range", type=float, default=2.5)
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp32"))
    ap.add_argument("--out", default="smooth")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/smooth_grid.py runs the model on an MI355X: no GPU here"
    import shot_vae_amd as S
    ch = 3 if a.kind == "svhn" else 1
    m = S.SmoothVAE((ch, 32, 32), {"cont": a.cont, "disc": [a.disc]}, kind=a.kind, compute_dtype=a.dtype)
    if a.state:
        m.load_state_dict(torch.load(a.state, map_location="cpu"))
    m = m.cuda().eval()
    Dd, n = a.disc, a.n
    samples, z = class_samples(m, n, a.key, a.tau)
    ext = ".ppm" if ch == 3 else ".pgm"
    save_grid(a.out + "_classes" + ext, samples, Dd, n)
    dims = [int(d) for d in a.dims.split(",") if d != ""]
    values = np.linspace(-a.range, a.range, a.steps).tolist()
    save_grid(a.out + "_traverse" + ext, traversal(m, dims, values), len(dims) * Dd, a.steps)
    sweep = m.traverse(z[::n].contiguous(), torch.arange(Dd, device="cuda"))           # the first sample of every class, re-rendered
    save_grid(a.out + "_class_sweep" + ext, sweep.flatten(0, 1), Dd, Dd)
    print("wrote %s_classes%s (%d x %d), %s_traverse%s (%d x %d) and %s_class_sweep%s (%d x %d)"
          % (a.out, ext, Dd, n, a.out, ext, len(dims) * Dd, a.steps, a.out, ext, Dd, Dd))


if __name__ == "__main__":
    main()
