"""Cost of dropout in the encoder (drop_rate 0.3 against 0) at the headline shape: WRN-28-2, B_l = B_u = 512, bf16, the grouped
step replayed as a hipGraph (GraphedTrainStep), both rates in one process; and the sv_dropout_fwd launch alone on the largest
tensor it sees in that step (conv1's output of the first stage, four groups of 512 x 32 x 32 x 32) -- bytes moved / time against
HBM.  Usage: python tools/dropout_bench.py [steps]"""
import ctypes
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shot_vae_amd as S                                   # noqa: E402
from shot_vae_amd import _lib as L                         # noqa: E402
from shot_vae_amd.train import GraphedTrainStep, schedule  # noqa: E402

NAME, K, B = "wideresnet-28-2", 10, 512


def step_ms(p, n):
    torch.manual_seed(0)
    m = S.VariationalAutoEncoder(NAME, num_input_channels=3, drop_rate=p, img_size=(32, 32), data_parallel=False,
                                 continuous_latent_dim=128, disc_latent_dim=K, small_input=True, compute_dtype="bf16",
                                 rng="device").cuda().train()
    elbo, cls = S.VAECriterion(discrete_dim=K).cuda(), S.ClsCriterion()
    opt = S.FlatSGD(m, lr=0.01)
    opt.zero_grad()
    il, ll = torch.rand(B, 3, 32, 32, device="cuda"), torch.randint(0, K, (B,), device="cuda")
    iu = torch.rand(B, 3, 32, 32, device="cuda")
    g = GraphedTrainStep(m, elbo, cls, opt, il, ll, iu, schedule(10), warmup=2)
    for _ in range(3):
        g()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        g()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def kernel_us(n=50):
    G, M, C = 4, B * 32 * 32, 32
    x = torch.randn(G, M, C, device="cuda").to(torch.bfloat16)
    keys = torch.randint(0, 2 ** 63 - 1, (G,), dtype=torch.int64, device="cuda")
    stats = torch.zeros(G * 32 * 2 * C, dtype=torch.float64, device="cuda")
    a = L.dropout_args(keys.data_ptr(), 0, 0.3)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch():
        L.call("sv_dropout_fwd", L.SV_BF16, ctypes.c_void_p(x.data_ptr()), M, C, C, ctypes.byref(a),
               ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(stats.data_ptr()), 32, G, st)

    for _ in range(5):
        launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        launch()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / n * 1e3
    return us, 2 * x.numel() * x.element_size()


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    t0, t3 = step_ms(0.0, n), step_ms(0.3, n)
    print("grouped step (hipGraph), %s, B_l = B_u = %d, bf16:  drop_rate 0: %.3f ms   drop_rate 0.3: %.3f ms   ratio %.3f"
          % (NAME, B, t0, t3, t3 / t0))
    us, nbytes = kernel_us()
    print("sv_dropout_fwd, 4 x %d x 32 x 32 x 32 bf16 in place: %.1f us, %.1f MB moved, %.2f TB/s"
          % (B, us, nbytes / 1e6, nbytes / us / 1e6))
