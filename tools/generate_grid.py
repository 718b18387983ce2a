"""Class-conditional image grids from a SHOT-VAE, written as binary PPM (PGM for one channel) with numpy alone:
  OUT_classes.ppm   K rows x n columns: row k = n samples of class k (VariationalAutoEncoder.generate, z ~ N(0, tau^2 I))
  OUT_analogy.ppm   one row per input image: the input, then its reconstruction under every class 0 .. K-1
                    (VariationalAutoEncoder.reconstruct(x, label=k): the posterior mean re-rendered under another class)
--state FILE: a state dict saved with torch.save (either data_parallel key layout); without it the default initialisation.
--images FILE.npy: uint8 [N, 32, 32, ch] input images for the analogy grid; without it the model's own first sample of each class.
Needs an MI355X.
Usage: python tools/generate_grid.py --encoder wideresnet-28-2 --classes 10 [--state FILE] [--images FILE.npy] [--n 8] [--tau 1.0]
                                     [--key 0] [--dtype bf16] [--out grid]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shot_vae_amd as S                                   # noqa: E402


def write_pnm(path, img):
    """img uint8 [H, W, ch], ch = 3 (P6) or 1 (P5)"""
    h, w, ch = img.shape
    assert img.dtype == np.uint8 and ch in (1, 3)
    with open(path, "wb") as f:
        f.write(b"%s\n%d %d\n255\n" % (b"P6" if ch == 3 else b"P5", w, h))
        f.write(np.ascontiguousarray(img).tobytes())


def tile(images, rows, cols, pad=2):
    """uint8 [rows * cols, H, W, ch] -> one uint8 image, row-major, `pad` white pixels between tiles"""
    n, h, w, ch = images.shape
    assert n == rows * cols
    out = np.full((rows * (h + pad) + pad, cols * (w + pad) + pad, ch), 255, dtype=np.uint8)
    for i in range(n):
        r, c = divmod(i, cols)
        out[pad + r * (h + pad): pad + r * (h + pad) + h, pad + c * (w + pad): pad + c * (w + pad) + w] = images[i]
    return out


def to_u8(img):
    """sigmoid images NCHW fp32 on the device -> uint8 NHWC numpy"""
    return (img.permute(0, 2, 3, 1) * 255.0 + 0.5).floor().clamp(0, 255).to(torch.uint8).cpu().numpy()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--encoder", default="wideresnet-28-2")
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--latent", type=int, default=128)
    ap.add_argument("--state")
    ap.add_argument("--images")
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--tau", type=float, default=1.0)
    ap.add_argument("--key", type=int, default=0)
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp32"))
    ap.add_argument("--out", default="grid")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/generate_grid.py runs the model on an MI355X: no GPU here"
    K, n = a.classes, a.n
    m = S.VariationalAutoEncoder(a.encoder, num_input_channels=a.channels, img_size=(32, 32), data_parallel=False,
                                 continuous_latent_dim=a.latent, disc_latent_dim=K, small_input=True, compute_dtype=a.dtype)
    if a.state:
        m.load_state_dict(torch.load(a.state, map_location="cpu"))
    m = m.cuda().eval()
    labels = torch.arange(K, device="cuda").repeat_interleave(n)            # row k = class k
    samples = m.generate(labels, a.key, tau=a.tau, dtype="uint8").cpu().numpy()
    write_pnm(a.out + "_classes.ppm", tile(samples, K, n))
    if a.images:
        src = np.load(a.images)
        assert src.dtype == np.uint8 and src.ndim == 4 and src.shape[1:] == (32, 32, a.channels), "--images: uint8 [N, 32, 32, ch]"
    else:
        src = samples[::n]                                                  # the first sample of every class
    x = torch.from_numpy(src).cuda().permute(0, 3, 1, 2).float().div(255.0).contiguous()
    cols = [src] + [to_u8(m.reconstruct(x, label=torch.full((len(src),), k, device="cuda"))) for k in range(K)]
    write_pnm(a.out + "_analogy.ppm", tile(np.stack(cols, axis=1).reshape((-1,) + src.shape[1:]), len(src), K + 1))
    print("wrote %s_classes.ppm (%d x %d) and %s_analogy.ppm (%d x %d)" % (a.out, K, n, a.out, len(src), K + 1))


if __name__ == "__main__":
    main()
