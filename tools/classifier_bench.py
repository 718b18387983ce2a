"""Step time of the classifier-only WideResNet baseline (shot_vae_amd/classifier.py) in bf16: classifier_train_step with FlatSGD,
issued eagerly and replayed as a hipGraph (GraphedClassifierStep), for wideresnet-28-2 (K = 10) and wideresnet-28-10 (K = 100) at
B = 128 (the reference's default batch, main_classifier.py:36) and B = 512.  After a warm-up every figure is the median of 7 timings of
20 back-to-back steps, with the spread (min .. max) beside it.  Fails without a GPU.

--trace NET B: twenty eager steps of one configuration on ONE stream and nothing else, for a kernel trace in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o cls -- python tools/classifier_bench.py --trace wideresnet-28-10 128
    python tools/kernel_stats_digest.py DIR/.../cls_kernel_stats.csv 20 "<header>"
--step-layers NET B: every launch of the eager step timed in place (HIP events around each launch, one stream, every kernel alone),
per layer: the tables profiles/classifier_*_step_layers.txt.
Usage: python tools/classifier_bench.py [--trace NET B | --step-layers NET B]"""
import ctypes
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shot_vae_amd as S                                   # noqa: E402
from shot_vae_amd import _lib as L                         # noqa: E402

CONFIGS = [("wideresnet-28-2", 10), ("wideresnet-28-10", 100)]
BATCHES = (128, 512)
REPS, N = 7, 20


def make(name, K, B):
    torch.manual_seed(0)
    m = S.get_wide_resnet(name, 0, input_channels=3, num_classes=K, small_input=True, data_parallel=False, compute_dtype="bf16")
    m = m.cuda().train()
    opt = S.FlatSGD(m, lr=0.01)
    opt.zero_grad()
    x, y = torch.rand(B, 3, 32, 32, device="cuda"), torch.randint(0, K, (B,), device="cuda")
    return m, S.CrossEntropyLoss(), opt, x, y


def timed_ms(step):
    for _ in range(5):
        step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        for _ in range(N):
            step()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / N * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def bench(name, K, B):
    m, crit, opt, x, y = make(name, K, B)
    eager = timed_ms(lambda: S.classifier_train_step(m, crit, opt, x, y))
    g = S.GraphedClassifierStep(m, crit, opt, x, y, warmup=2)
    graph = timed_ms(g)
    loss = float(g())
    assert loss == loss, "NaN loss"
    for label, (med, lo, hi) in (("eager", eager), ("hipGraph", graph)):
        print("classifier step, %s, K = %d, B = %d, bf16, %-8s: %.3f ms  (min %.3f .. max %.3f)  %.0f images/s"
              % (name, K, B, label, med, lo, hi, B / med * 1e3))


def trace(name, K, B):
    m, crit, opt, x, y = make(name, K, B)
    m._engine.wgrad_side_stream = False          # one stream: the side stream's concurrent weight gradients would inflate the durations
    for _ in range(N):
        S.classifier_train_step(m, crit, opt, x, y)
    torch.cuda.synchronize()


def step_layers(name, K, B, steps=3):
    """per-layer times of the eager step (the in-situ timing pass of bench.py --full, for this network)"""
    m, crit, opt, x, y = make(name, K, B)
    for _ in range(2):
        S.classifier_train_step(m, crit, opt, x, y)
    torch.cuda.synchronize()
    eng = m._engine
    eng.prof_tags, eng.prof_cost = {}, {}
    L.prof_tags = eng.prof_tags
    L.lib().sv_prof_nested_tag(eng.prof_tags.setdefault("sv_bn_finalize(folded)", len(eng.prof_tags)))
    L.lib().sv_prof_enable(1)
    side, eng.wgrad_side_stream = eng.wgrad_side_stream, False
    try:
        for _ in range(steps):
            S.classifier_train_step(m, crit, opt, x, y)
        ntag = len(eng.prof_tags) + 1
        ms, cnt = (ctypes.c_double * ntag)(), (ctypes.c_int * ntag)()
        L.lib().sv_prof_collect(ntag, ms, cnt)
    finally:
        L.lib().sv_prof_enable(0)
        L.lib().sv_prof_nested_tag(-1)
        tags, cost = dict(eng.prof_tags), dict(eng.prof_cost)
        L.prof_tags = eng.prof_tags = None
        eng.wgrad_side_stream = side
    print("eager classifier step of %s, K = %d, B = %d, bf16: every launch timed alone, %d steps" % (name, K, B, steps))
    print("  %-34s %9s %9s %11s %9s" % ("launch", "per step", "avg us", "ms / step", "TFLOP/s"))
    rows = sorted(((ms[i] / steps, n, cnt[i] // steps, 1e3 * ms[i] / max(cnt[i], 1)) for n, i in tags.items() if cnt[i]), reverse=True)
    for tot, n, per, avg in rows:
        _, flops, nl = cost.get(n, (0.0, 0.0, 0))
        tf = "%9.0f" % (flops / nl / avg / 1e6) if nl and flops else "%9s" % "-"
        print("  %-34s %9d %9.1f %11.3f %s" % (n, per, avg, tot, tf))
    print("  %-34s %9s %9s %11.3f" % ("sum", "", "", sum(r[0] for r in rows)))


if __name__ == "__main__":
    assert torch.cuda.is_available(), "tools/classifier_bench.py measures on an MI355X: no GPU here"
    if len(sys.argv) > 1 and sys.argv[1] in ("--trace", "--step-layers"):
        name, B = sys.argv[2], int(sys.argv[3])
        K = dict(CONFIGS)[name]
        (trace if sys.argv[1] == "--trace" else step_layers)(name, K, B)
        sys.exit(0)
    for name, K in CONFIGS:
        for B in BATCHES:
            bench(name, K, B)
