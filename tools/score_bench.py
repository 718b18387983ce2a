"""Timings of the per-image scores of the SHOT-VAE on wideresnet-28-2, K = 10, B = 512 images, bf16, S = 1 and S = 16 samples:
  score                 VariationalAutoEncoder.score(x, criterion, samples=S, key): the four ELBO terms per image, eager
  log_likelihood        VariationalAutoEncoder.log_likelihood(x, criterion, S, key): the importance-weighted bound, eager
  *-graph               the same call captured once into a hipGraph and replayed with a new key
  split                 one in-situ timed pass (HIP events around every launch) of log_likelihood: kernel time of the encoder and its
                        heads / sv_latent_sweep / the decoder / sv_recon_rows + sv_score_reduce, with each part's share.  The events
                        keep launches from overlapping and cost time themselves: the sum exceeds the call time of the timed items
  public-api            the yardstick: the same quantities through the calls the package had before -- encode, a Python loop of decode
                        over samples and classes (z drawn with torch), torch's binary_cross_entropy_with_logits sums per image and
                        logsumexp -- recon, kl_c, kl_d, elbo and log_px of every image
Both paths decode B * S * K = 5120 * S latents.  One thing per process: the driver starts a fresh child for every item, one after
the other, and stops at the first that fails.  In a child: 3 warm-up calls, then the median of 5 timings of n back-to-back calls that
end in a device synchronise (n: at least 3, and enough for a quarter of a second per timing), with the spread beside it.  There is
no target: the figures are a record (profiles/score_bench.txt).  Fails without a GPU.
Usage: python tools/score_bench.py [--one ITEM S]"""
import ctypes
import math
import os
import statistics
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shot_vae_amd as S                                   # noqa: E402
from shot_vae_amd import _lib as L                         # noqa: E402

NAME, K, B = "wideresnet-28-2", 10, 512
SAMPLES = (1, 16)
ITEMS = ("score", "score-graph", "log_likelihood", "log_likelihood-graph", "split", "public-api")
REPS, N, WINDOW_S = 5, 3, 0.25


def timed_ms(call):
    for _ in range(3):
        call()
    torch.cuda.synchronize()

    def window(n):
        t0 = time.perf_counter()
        for _ in range(n):
            call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    n = max(N, min(2000, int(WINDOW_S / window(N)) + 1))
    ts = [window(n) * 1e3 for _ in range(REPS)]
    return statistics.median(ts), min(ts), max(ts), n


def public_api(m, x, samples, gen):
    """what a user of the package's earlier calls writes: per-image recon / kl_c / kl_d / elbo / log_px"""
    mu, ls, la = m.encode(x)
    q, sd = la.exp(), ls.exp()
    nll = torch.empty(B, samples, K, device=x.device)
    lw = torch.empty(B, samples, device=x.device)
    for s in range(samples):
        n = torch.randn(B, mu.size(1), device=x.device, generator=gen)
        z = mu + sd * n
        lw[:, s] = (0.5 * n * n - 0.5 * z * z + ls).sum(dim=1)
        for k in range(K):
            rec = m.decode(z, torch.full((B,), k, dtype=torch.int64, device=x.device))
            nll[:, s, k] = torch.nn.functional.binary_cross_entropy_with_logits(rec, x, reduction="none").sum(dim=(1, 2, 3))
    recon = (q[:, None, :] * nll).sum(dim=(1, 2)) / samples
    kl_c = 0.5 * (mu * mu + torch.exp(2 * ls) - 2 * ls - 1).sum(dim=1)
    kl_d = (q * (la + math.log(K))).sum(dim=1)
    log_px = torch.logsumexp(lw + torch.logsumexp(-nll - math.log(K), dim=2), dim=1) - math.log(samples)
    return recon, kl_c, kl_d, -(recon + kl_c + kl_d), log_px


def graphed(fn, key):
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fn()
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
        out = fn()

    def call():
        key.add_(1)
        graph.replay()
        return out
    return call


def split(m, fn, x):
    """kernel ms of one call of fn by part, from the in-situ timing of every launch; the encoder's part is that of an encode(x)"""
    eng = m._engine

    def prof(call):
        eng.prof_tags, eng.prof_cost = {}, {}
        L.prof_tags = eng.prof_tags
        L.lib().sv_prof_enable(1)
        try:
            call()
            torch.cuda.synchronize()
            ntag = len(eng.prof_tags) + 1
            ms, cnt = (ctypes.c_double * ntag)(), (ctypes.c_int * ntag)()
            L.lib().sv_prof_collect(ntag, ms, cnt)
            return {name: ms[i] for name, i in eng.prof_tags.items() if cnt[i]}
        finally:
            L.lib().sv_prof_enable(0)
            L.prof_tags = eng.prof_tags = None
    fn()
    torch.cuda.synchronize()
    enc = sum(prof(lambda: m.encode(x)).values())
    t = prof(fn)
    sweep, red = t.get("sv_latent_sweep", 0.0), t.get("sv_recon_rows", 0.0) + t.get("sv_score_reduce", 0.0)
    return enc, sweep, sum(t.values()) - enc - sweep - red, red


def one(item, samples):
    torch.manual_seed(0)
    m = S.VariationalAutoEncoder(NAME, num_input_channels=3, img_size=(32, 32), data_parallel=False, continuous_latent_dim=128,
                                 disc_latent_dim=K, small_input=True, compute_dtype="bf16", rng="device").cuda().eval()
    crit = S.VAECriterion(discrete_dim=K)
    x = torch.rand(B, 3, 32, 32, device="cuda")
    key = torch.tensor([1], dtype=torch.int64, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(1)
    head = "%-15s K = %d, B = %d, bf16, S = %2d, %-20s:" % (NAME, K, B, samples, item)
    fns = {"score": lambda: m.score(x, crit, samples=samples, key=key), "log_likelihood": lambda: m.log_likelihood(x, crit, samples, key),
           "public-api": lambda: public_api(m, x, samples, gen)}
    if item == "split":
        enc, sweep, dec, red = split(m, fns["log_likelihood"], x)
        tot = enc + sweep + dec + red
        print("%s profiled pass, kernel ms (share): encode %.3f (%.0f%%), sweep %.3f (%.0f%%), decoder %.3f (%.0f%%), reduction %.3f (%.0f%%); "
              "sum %.3f, more than the call time" % (head, enc, 100 * enc / tot, sweep, 100 * sweep / tot, dec, 100 * dec / tot, red,
                                                     100 * red / tot, tot), flush=True)
        return
    call = graphed(fns[item[:-6]], key) if item.endswith("-graph") else fns[item]
    med, lo, hi, n = timed_ms(call)
    res = call()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in (res if isinstance(res, tuple) else (res,)))
    print("%s %9.3f ms  (min %.3f .. max %.3f; %d x %4d calls)  %9.0f images/s" % (head, med, lo, hi, REPS, n, B / med * 1e3), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "tools/score_bench.py measures on an MI355X: no GPU here"
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(sys.argv[2], int(sys.argv[3]))
        sys.exit(0)
    for samples in SAMPLES:
        for item in ITEMS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", item, str(samples)], timeout=300)
            if r.returncode != 0:
                sys.exit("tools/score_bench.py: %s S=%d failed (exit status %d); nothing further was started" % (item, samples, r.returncode))
