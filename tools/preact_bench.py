"""PreActResNet-18 at B_l = B_u = 512 in bf16: the grouped step replayed as a hipGraph (GraphedTrainStep), and the 512 -> 512 3x3 layer
of its last stage alone (4 x 4 maps, 4 x 512 images = the four groups of the step) in forward, data gradient and weight gradient,
with the 4 x 4-map instantiations on and off: wgrad3x3's is on by default (SV_K_MAP4 in SV_OPT_DISABLE_MASK switches it off),
conv3x3's (forward / data gradient) is off by default (SV_K_MAP4_CONV in SV_OPT_ENABLE_MASK switches it on); "general path" = the
gather-GEMM / general weight-gradient kernels, which these layers took before.  Each figure is the median of `reps` timings of `n` back-to-back
launches, with the spread (min .. max) beside it.
--general-only: the layer on the general path alone, no step (for a kernel trace of exactly that path: run it under
`rocprofv3 --kernel-trace --stats -- python tools/preact_bench.py --general-only`, also with SV_LIB_PATH pointing at a build of an
earlier commit, and compare the kernel names).  --step-layers: every launch of one eager grouped step timed in place (HIP events
around each launch, the engine's profiling tags: one stream, every kernel alone), per layer.
Usage: python tools/preact_bench.py [steps] [--layers-only | --general-only | --step-layers]"""
import ctypes
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shot_vae_amd as S                                   # noqa: E402
from shot_vae_amd import _lib as L                         # noqa: E402
from shot_vae_amd import geometry as G                     # noqa: E402
from shot_vae_amd.train import GraphedTrainStep, schedule  # noqa: E402

NAME, K, B = "preactresnet18", 10, 512


def step_ms(n, dis=0, en=0):
    torch.manual_seed(0)
    with L.options(disable=dis, enable=en):
        m = S.VariationalAutoEncoder(NAME, num_input_channels=3, drop_rate=0, img_size=(32, 32), data_parallel=False,
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
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(n):
                g()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / n * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def timed(launch, n=20, reps=7):
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            launch()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) / n * 1e3)
    return statistics.median(us), min(us), max(us)


def step_layers(steps=3):
    """per-layer times of the eager grouped step (the in-situ timing pass of bench.py --full, for this network)"""
    from shot_vae_amd.train import train_step_grouped
    torch.manual_seed(0)
    m = S.VariationalAutoEncoder(NAME, num_input_channels=3, drop_rate=0, img_size=(32, 32), data_parallel=False,
                                 continuous_latent_dim=128, disc_latent_dim=K, small_input=True, compute_dtype="bf16",
                                 rng="device").cuda().train()
    elbo, cls = S.VAECriterion(discrete_dim=K).cuda(), S.ClsCriterion()
    opt = S.FlatSGD(m, lr=0.01)
    opt.zero_grad()
    il, ll = torch.rand(B, 3, 32, 32, device="cuda"), torch.randint(0, K, (B,), device="cuda")
    iu = torch.rand(B, 3, 32, 32, device="cuda")
    sch = schedule(10)
    for _ in range(2):
        train_step_grouped(m, elbo, cls, opt, il, ll, iu, sch)
    torch.cuda.synchronize()
    eng = m._engine
    eng.prof_tags, eng.prof_cost = {}, {}
    L.prof_tags = eng.prof_tags
    L.lib().sv_prof_nested_tag(eng.prof_tags.setdefault("sv_bn_finalize(folded)", len(eng.prof_tags)))
    L.lib().sv_prof_enable(1)
    side, eng.wgrad_side_stream = eng.wgrad_side_stream, False
    try:
        for _ in range(steps):
            train_step_grouped(m, elbo, cls, opt, il, ll, iu, sch)
        ntag = len(eng.prof_tags) + 1
        ms, cnt = (ctypes.c_double * ntag)(), (ctypes.c_int * ntag)()
        L.lib().sv_prof_collect(ntag, ms, cnt)
    finally:
        L.lib().sv_prof_enable(0)
        L.lib().sv_prof_nested_tag(-1)
        tags, cost = dict(eng.prof_tags), dict(eng.prof_cost)
        L.prof_tags = eng.prof_tags = None
        eng.wgrad_side_stream = side
    print("eager grouped step of %s, B_l = B_u = %d, bf16: every launch timed alone, %d steps; layers = convolution launches of "
          "four groups x %d images" % (NAME, B, steps, B))
    print("  %-34s %9s %9s %11s %9s" % ("launch", "per step", "avg us", "ms / step", "TFLOP/s"))
    rows = sorted(((ms[i] / steps, n, cnt[i] // steps, 1e3 * ms[i] / max(cnt[i], 1)) for n, i in tags.items() if cnt[i]), reverse=True)
    for tot, n, per, avg in rows:
        _, flops, nl = cost.get(n, (0.0, 0.0, 0))
        tf = "%9.0f" % (flops / nl / avg / 1e6) if nl and flops else "%9s" % "-"
        print("  %-34s %9d %9.1f %11.3f %s" % (n, per, avg, tot, tf))
    print("  %-34s %9s %9s %11.3f" % ("sum", "", "", sum(r[0] for r in rows)))


def layer_us(Gn=4, C=512, general_only=False):
    d = "cuda"
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    bf = torch.bfloat16
    x = torch.randn(Gn * B, 4, 4, C, device=d).to(bf)
    dy = torch.randn(Gn * B, 4, 4, C, device=d).to(bf)
    out = torch.empty_like(x)
    sc, sh = torch.rand(Gn, C, device=d) + 0.5, torch.randn(Gn, C, device=d) * 0.3
    mean, rstd = torch.randn(Gn, C, device=d) * 0.1, torch.rand(Gn, C, device=d) + 0.5
    master = (torch.randn(C, 9, C, device=d) / (9 * C) ** 0.5).contiguous()
    gf, gd = G.conv_like(B, 4, 4, C, C, 3, 1, 1), G.convT_like(B, 4, 4, C, C, 3, 1, 1)
    packs = []
    for g, tr in ((gf, 0), (gd, 1)):
        pk = torch.zeros(G.packed_size(g), dtype=bf, device=d)
        L.call("sv_repack", L.SV_BF16, ctypes.c_void_p(master.data_ptr()), C, 9, C, tr, ctypes.byref(g), ctypes.c_void_p(pk.data_ptr()), st)
        packs.append(pk)
    stats = torch.zeros(Gn * 4 * 2 * C, dtype=torch.float64, device=d)
    dw = torch.zeros(C, 9, C, device=d)
    ws = torch.empty(16 * 1024 * 1024, device=d)

    def fwd():
        a = L.SvIgemmArgs()
        a.x, a.w, a.out, a.groups, a.replicas = x.data_ptr(), packs[0].data_ptr(), out.data_ptr(), Gn, 4
        a.pro_scale, a.pro_shift, a.pro_slope = sc.data_ptr(), sh.data_ptr(), 0.0
        a.residual, a.stats = dy.data_ptr(), stats.data_ptr()
        L.call("sv_igemm", ctypes.byref(gf), L.SV_BF16, ctypes.byref(a), st)

    def dgrad():
        a = L.SvIgemmArgs()
        a.x, a.w, a.out, a.groups, a.replicas = dy.data_ptr(), packs[1].data_ptr(), out.data_ptr(), Gn, 4
        a.ex, a.ex_scale, a.ex_shift, a.ex_mean, a.ex_rstd = x.data_ptr(), sc.data_ptr(), sh.data_ptr(), mean.data_ptr(), rstd.data_ptr()
        a.ex_slope, a.bsums = 0.0, stats.data_ptr()
        L.call("sv_igemm", ctypes.byref(gd), L.SV_BF16, ctypes.byref(a), st)

    def wgrad():
        a = L.SvWgradArgs()
        a.x, a.dy, a.dw = x.data_ptr(), dy.data_ptr(), dw.data_ptr()
        a.pro_scale, a.pro_shift, a.pro_slope = sc.data_ptr(), sh.data_ptr(), 0.0
        a.splits, a.use_tr, a.ws, a.ws_elems, a.groups, a.block_budget = 0, 1, ws.data_ptr(), ws.numel(), Gn, 0
        L.call("sv_wgrad_ex", ctypes.byref(gf), L.SV_BF16, ctypes.byref(a), st)

    flops = 2.0 * Gn * B * 16 * C * 9 * C
    print("layer 512 -> 512, 3x3 stride 1 on 4 x 4 maps, %d x %d images, bf16: 2*M*N*K = %.1f GFLOP, weights %.2f MB (bf16), "
          "activations %.1f MB per tensor" % (Gn, B, flops / 1e9, 9 * C * C * 2 / 1e6, x.numel() * 2 / 1e6))
    for name, fn in (("forward", fwd), ("data gradient", dgrad), ("weight gradient", wgrad)):
        for label, dis, en in (("4x4 instantiation", 0, L.K_MAP4_CONV), ("general path", L.K_MAP4, 0)):
            if general_only and not dis:
                continue
            with L.options(disable=dis, enable=en):
                med, lo, hi = timed(fn)
            print("  %-16s %-20s %8.1f us  (min %.1f .. max %.1f)  %.0f TFLOP/s" % (name, label, med, lo, hi, flops / med / 1e6))


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if args else 10
    if "--step-layers" in sys.argv:
        step_layers()
        sys.exit(0)
    layer_us(general_only="--general-only" in sys.argv)
    if "--layers-only" not in sys.argv and "--general-only" not in sys.argv:
        for label, dis, en in (("default (4x4 weight gradient on)", 0, 0), ("all 4x4 instantiations on", 0, L.K_MAP4_CONV),
                               ("all off (the general kernels)", L.K_MAP4, 0)):
            med, lo, hi = step_ms(n, dis, en)
            print("grouped step (hipGraph), %s, B_l = B_u = %d, bf16, %s: %.3f ms  (min %.3f .. max %.3f)" % (NAME, B, label, med, lo, hi))
