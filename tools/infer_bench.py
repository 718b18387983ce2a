"""Inference timings of the SHOT-VAE in bf16 at B = 512 on wideresnet-28-2 (K = 10) and wideresnet-28-10 (K = 100):
  forward         the eval model(x) that encode replaces (encoder, heads, sampler, decoder, the reconstruction's NCHW copy)
  encode          VariationalAutoEncoder.encode(x): encoder + heads only
  generate        VariationalAutoEncoder.generate(labels, key) with a device key, issued eagerly: images / s
  generate-graph  the same call captured once into a hipGraph and replayed: images / s
One thing per process: the driver starts a fresh child for every (network, item), one after the other, and stops at the first that
fails.  In a child: 5 warm-up calls, then the median of 7 timings of n back-to-back calls that end in a device synchronise (n: at
least 20, and enough for a quarter of a second per timing), with the spread (min .. max) beside it.  There is no target: the
figures are a record (profiles/infer_bench.txt).  Fails without a GPU.
Usage: python tools/infer_bench.py [--one NET ITEM]"""
import os
import statistics
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shot_vae_amd as S                                   # noqa: E402

CONFIGS = [("wideresnet-28-2", 10), ("wideresnet-28-10", 100)]
ITEMS = ("forward", "encode", "generate", "generate-graph")
B, REPS, N, WINDOW_S = 512, 7, 20, 0.25


def timed_ms(call):
    for _ in range(5):
        call()
    torch.cuda.synchronize()

    def window(n):
        t0 = time.perf_counter()
        for _ in range(n):
            call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    n = max(N, min(5000, int(WINDOW_S / window(N)) + 1))      # a window of a few ms would time the clock and the scheduler
    ts = [window(n) * 1e3 for _ in range(REPS)]
    return statistics.median(ts), min(ts), max(ts), n


def one(name, item):
    K = dict(CONFIGS)[name]
    torch.manual_seed(0)
    m = S.VariationalAutoEncoder(name, num_input_channels=3, img_size=(32, 32), data_parallel=False, continuous_latent_dim=128,
                                 disc_latent_dim=K, small_input=True, compute_dtype="bf16", rng="device").cuda().eval()
    x = torch.rand(B, 3, 32, 32, device="cuda")
    labels = torch.randint(0, K, (B,), device="cuda")
    key = torch.tensor([1], dtype=torch.int64, device="cuda")
    if item == "forward":
        def call():
            with torch.no_grad():
                return m(x)
    elif item == "encode":
        call = lambda: m.encode(x)
    elif item == "generate":
        call = lambda: m.generate(labels, key)
    else:
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            m.generate(labels, key)
        torch.cuda.current_stream().wait_stream(stream)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
            out = m.generate(labels, key)

        def call():
            key.add_(1)
            graph.replay()
            return out
    med, lo, hi, n = timed_ms(call)
    res = call()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in (res if isinstance(res, tuple) else (res,)))
    print("%-16s K = %3d, B = %d, bf16, %-14s: %8.3f ms  (min %.3f .. max %.3f; 7 x %4d calls)  %9.0f images/s"
          % (name, K, B, item, med, lo, hi, n, B / med * 1e3), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "tools/infer_bench.py measures on an MI355X: no GPU here"
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(sys.argv[2], sys.argv[3])
        sys.exit(0)
    for name, _ in CONFIGS:
        for item in ITEMS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, item], timeout=300)
            if r.returncode != 0:
                sys.exit("tools/infer_bench.py: %s %s failed (exit status %d); nothing further was started" % (name, item, r.returncode))
