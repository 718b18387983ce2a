"""The six launches of the decoder's first three ConvTranspose2d(4, 2, 1) layers, alone, at the headline step's sizes: forward on
4 x 512 images (four BatchNorm groups, materialised input, statistics epilogue) and data gradient on 2 x 512 (activation-backward
epilogue), with the per-pixel GEMM kernel (pixgemm.hip) switched off and on.

    python tools/probes/decoder_gemm_layers.py [B]

Prints one row per launch: microseconds with SV_K_PIXGEMM disabled / enabled, the kernel each took, and the floors of the valid
taps at 2.5 PFLOP/s and of the operand bytes at 8 TB/s."""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from shot_vae_amd import _lib as L          # noqa: E402
from shot_vae_amd import geometry as G      # noqa: E402
from shot_vae_amd.engine import _replicas   # noqa: E402

LAYERS = [("dec1", 1, 1024, 512), ("dec2", 2, 512, 256), ("dec3", 4, 256, 128)]      # name, Hin, Cin, N
PAIRS = {1: 4, 2: 36, 4: 196}                                                        # valid (pixel, tap) pairs of the layer


def timed(fn, iters=50, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def launches(B):
    d, bf = torch.device("cuda:0"), torch.bfloat16
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    keep = []
    for name, H, Cin, N in LAYERS:
        Ho = 2 * H
        master = (torch.randn(N, 16, Cin, device=d) / (4 * Cin) ** 0.5).contiguous()
        for kind, groups in (("fwd", 4), ("dgrad", 2)):
            if kind == "fwd":
                g, cin, n, hi, ho = G.convT_like(B, H, H, Cin, N, 4, 2, 1), Cin, N, H, Ho
            else:
                g, cin, n, hi, ho = G.conv_like(B, Ho, Ho, N, Cin, 4, 2, 1), N, Cin, Ho, H
            wp = torch.zeros(G.packed_size(g), dtype=bf, device=d)
            L.call("sv_repack", L.SV_BF16, C.c_void_p(master.data_ptr()), N, 16, Cin, int(kind == "dgrad"), C.byref(g), C.c_void_p(wp.data_ptr()), st)
            x = torch.randn(groups * B, hi, hi, cin, device=d).to(bf)
            out = torch.empty(groups * B, ho, ho, n, dtype=bf, device=d)
            R = _replicas(B * ho * ho)
            acc = torch.zeros(groups, R, 2 * n, device=d, dtype=torch.float64)
            a = L.SvIgemmArgs()
            a.x, a.w, a.out, a.groups, a.replicas = x.data_ptr(), wp.data_ptr(), out.data_ptr(), groups, R
            if kind == "fwd":
                a.stats = acc.data_ptr()
            else:
                raw = torch.randn(groups * B, ho, ho, n, device=d).to(bf)
                vec = [torch.rand(groups, n, device=d) + 0.5 for _ in range(4)]
                a.ex, a.ex_scale, a.ex_shift, a.ex_mean, a.ex_rstd = [t.data_ptr() for t in [raw] + vec]
                a.ex_slope, a.bsums = 0.0, acc.data_ptr()
                keep += [raw, vec]
            keep += [wp, x, out, acc, master]
            flops = 2.0 * groups * B * PAIRS[H] * Cin * N
            by = 2.0 * (x.numel() + out.numel() * (2 if kind == "dgrad" else 1) + wp.numel())
            yield name, kind, groups, g, a, st, flops / 2.5e15 * 1e6, by / 8e12 * 1e6


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    print("%-11s %6s %10s %10s  %-16s %-16s %9s %9s" % ("launch", "images", "off, us", "on, us", "kernel off", "kernel on", "MFMA, us", "HBM, us"))
    for name, kind, groups, g, a, st, f_mfma, f_hbm in launches(B):
        res = []
        for mask in (L.K_PIXGEMM, 0):
            with L.options(disable=mask):
                us = timed(lambda: L.call("sv_igemm", C.byref(g), L.SV_BF16, C.byref(a), st))
                res.append((us, L.last_kernel()))
        print("%-11s %6s %10.1f %10.1f  %-16s %-16s %9.1f %9.1f" % (kind + " " + name, "%dx%d" % (groups, B), res[0][0], res[1][0], res[0][1], res[1][1],
                                                                   f_mfma, f_hbm), flush=True)


if __name__ == "__main__":
    main()
