"""The aggregate-posterior density at a fixed shape -- Q = 10 000 sampled latents, N = 50 000 gallery posteriors, D = 128 -- two ways:
  fused   AggregatePosterior.log_density: sv_aggpost_scan (the joint density) / sv_aggpost_dims (the per-dimension marginals), each
          followed by sv_aggpost_finish; no [Q, N] or [Q, N, D] array exists
  torch   torch.logsumexp over the broadcast [chunk, N, D] expression in the style of lib/utils/calculate_dist.py, over chunks of CHUNK
          query rows -- each of its [chunk, N, D] intermediates is 1.6 GB at CHUNK = 64
One item ("scan" or "dims") per process: the driver starts a fresh child for each, one after the other, and stops at the first that
fails.  In a child both ways run in the same process state, each after its own warm-up: fused 3 warm-up passes and the median of 7
timings of 5 back-to-back passes, torch 1 warm-up pass and the median of 3 single passes (a pass takes seconds).  Every timing ends in a
device synchronise.  The child asserts that the two agree to 1e-3.  The "scan" child also times LatentIndex.search(k = 1, "kl") on the
same rows in the same process -- the same arithmetic per pair, with a 1-slot list where the log-sum-exp state is -- and prints the ratio:
information, not a bar.  The bar: neither fused pass is slower than its torch formulation (profiles/aggpost_bench.txt).  Fails without a
GPU.
Usage: python tools/aggpost_bench.py [--out profiles/aggpost_bench.txt] [--items scan,dims] | --one ITEM"""
import argparse
import math
import os
import re
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shot_vae_amd as S                                   # noqa: E402
from tools.knn_bench import timed_ms                       # noqa: E402

Q, N, D, CHUNK = 10000, 50000, 128, 64
ITEMS = ("scan", "dims")


def torch_density(z, mu, ls, per_dim, out):
    """log 1/N sum_j N(z_i; mu_j, sigma_j^2) (per_dim: of every dimension on its own), chunked over the query rows"""
    iv = 1.0 / torch.exp(ls) ** 2
    for a in range(0, z.shape[0], CHUNK):
        lp = -0.5 * (torch.unsqueeze(z[a:a + CHUNK], 1) - torch.unsqueeze(mu, 0)) ** 2 * torch.unsqueeze(iv, 0) \
            - torch.unsqueeze(ls, 0) - 0.5 * math.log(2.0 * math.pi)
        out[a:a + CHUNK] = torch.logsumexp(lp if per_dim else torch.sum(lp, dim=2), dim=1) - math.log(mu.shape[0])
    return out


def one(item):
    g = torch.Generator(device="cuda").manual_seed(0)
    # nearly coincident posteriors (the `overlap` recipe of tests/_aggpost_ref.py): many gallery rows carry every sum
    base = torch.rand(1, D, device="cuda", generator=g) * 1.5 - 1.0
    ls = base + 0.01 * (torch.rand(N, D, device="cuda", generator=g) * 2.0 - 1.0)
    mu = 0.1 * torch.exp(base) * torch.randn(N, D, device="cuda", generator=g)
    agg = S.AggregatePosterior(D)
    agg.add(mu, ls)
    z = agg.sample(mu[:Q], ls[:Q], key=1)[0]
    per_dim = item == "dims"
    ref = torch.empty((Q, D) if per_dim else (Q,), dtype=torch.float32, device="cuda")

    def fused():
        return agg.log_density(z)

    def fused_dims_only():                                  # the dims pass without the scan log_density(per_dim=True) also runs
        state = torch.empty(2, P, Q * D, dtype=torch.float64, device="cuda")
        out = torch.empty(Q * D, dtype=torch.float32, device="cuda")
        L, p, st = S.aggregate.L, S.aggregate._p, S.aggregate._st
        L.call("sv_aggpost_dims", p(z), Q, p(agg.index.mu), p(agg.index.ls), N, D, 0, -1, p(state[0]), p(state[1]), P, 1, st())
        L.call("sv_aggpost_finish", p(state[0]), p(state[1]), P, Q * D, N, p(out), st())
        return out.view(Q, D)

    P = S.aggregate.partials(-(-Q // 32) * -(-D // 64), N) if per_dim else S.aggregate.partials(-(-Q // 64), N)
    call = fused_dims_only if per_dim else fused
    err = float((call() - torch_density(z, mu, ls, per_dim, ref)).abs().max())
    assert err <= 1e-3, "fused and torch disagree: %g" % err
    rows = []
    runs = [("fused", call, 3, 7, 5), ("torch", lambda: torch_density(z, mu, ls, per_dim, ref), 1, 3, 1)]
    if not per_dim:
        index = agg.index
        runs.append(("search k=1 kl", lambda: index.search(z, ls[:Q], 1), 3, 7, 5))
    for name, fn, warm, reps, n in runs:
        med, lo, hi = timed_ms(fn, warm, reps, n)
        rows.append(med)
        print("%-4s P=%2d  %-13s: %10.3f ms  (min %.3f .. max %.3f; %d x %d passes)" % (item, P, name, med, lo, hi, reps, n), flush=True)
    print("%-4s torch / fused = %.2f   max |fused - torch| = %.1e" % (item, rows[1] / rows[0], err), flush=True)
    if not per_dim:
        print("%-4s fused / search(k = 1, kl) = %.2f" % (item, rows[0] / rows[2]), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "tools/aggpost_bench.py measures on an MI355X: no GPU here"
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(sys.argv[2])
        sys.exit(0)
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "aggpost_bench.txt"))
    ap.add_argument("--items", default=",".join(ITEMS))
    a = ap.parse_args()
    lines = ["aggregate-posterior density, Q = %d, N = %d, D = %d, fp32, %s (tools/aggpost_bench.py)" % (Q, N, D, torch.cuda.get_device_name(0))]
    print(lines[0], flush=True)
    slower = []
    for item in a.items.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", item], timeout=600, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        sys.stderr.write(r.stderr[-2000:])
        lines += r.stdout.splitlines()
        if r.returncode != 0:
            sys.exit("tools/aggpost_bench.py: %s failed (exit status %d); nothing further was started" % (item, r.returncode))
        if float(re.search(r"torch / fused = ([0-9.]+)", r.stdout).group(1)) < 1.0:
            slower.append(item)
    lines.append("the bar (neither fused pass slower than its torch formulation): %s" % ("MISSED for " + ", ".join(slower) if slower else "met"))
    print(lines[-1])
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
