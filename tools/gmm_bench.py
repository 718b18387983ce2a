"""One EM iteration of a diagonal Gaussian mixture at a fixed shape -- N = 50 000 rows, D = 128, K = 10 / 100 components -- two ways:
  fused   sv_gmm_estep + sv_gmm_accum + sv_gmm_finish (shot_vae_amd.mixture.GaussianMixture.step): no [N, K] matrix exists, no atomic,
          the same bits every time
  torch   the matmul-expanded log-densities (x^2 @ ivar^T - 2 x @ (mean ivar)^T + sum mean^2 ivar), logsumexp, resp^T @ x and
          resp^T @ x^2 and scikit-learn's M-step: stores the [N, K] matrix twice
each eager and replayed from a captured graph (torch.cuda.graph), plus the three fused launches timed on their own (what bounds ours).
One item (a K) per process: the driver starts a fresh child for each, one after the other, and stops at the first that fails.  In a
child every way starts every pass from the SAME parameters (a copy back, inside the timed region of both ways) and runs in the same
process state after its own warm-up (3 passes): the median of 7 timings of 20 back-to-back passes, each timing ending in a device
synchronise.  The child prints the largest difference between the two sets of parameters after one iteration.  No ratio is required:
the file records what was measured (profiles/gmm_bench.txt).  Fails without a GPU.
Usage: python tools/gmm_bench.py [--out profiles/gmm_bench.txt] [--items 10,100] | --one K"""
import argparse
import math
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shot_vae_amd as S                                   # noqa: E402
from shot_vae_amd import mixture as MX                     # noqa: E402
from tools.cluster_bench import graphed                    # noqa: E402
from tools.knn_bench import timed_ms                       # noqa: E402

N, D = 50000, 128
ITEMS = ("10", "100")
WARM, REPS, PASSES = 3, 7, 20
REG = 1e-6


def torch_step(x, x2, logw, mean, var):
    ivar = 1.0 / var
    q = x2 @ ivar.t() - 2.0 * (x @ (mean * ivar).t()) + (mean * mean * ivar).sum(dim=1)[None, :]
    v = (logw - 0.5 * (D * math.log(2.0 * math.pi) + var.log().sum(dim=1)))[None, :] - 0.5 * q
    lse = torch.logsumexp(v, dim=1)
    resp = (v - lse[:, None]).exp()
    nk = resp.sum(dim=0) + 10.0 * torch.finfo(torch.float64).eps
    m = (resp.t() @ x) / nk[:, None]
    s = (resp.t() @ x2) / nk[:, None] - m * m + REG
    return (nk / nk.sum()).log(), m, s, lse.mean()


def one(K):
    g = torch.Generator(device="cuda").manual_seed(0)
    centres = 3.0 * torch.randn(K, D, device="cuda", generator=g)
    x = (centres[torch.randint(0, K, (N,), device="cuda", generator=g)] + torch.randn(N, D, device="cuda", generator=g)).contiguous()
    x2 = x * x
    m0 = x[torch.randperm(N, device="cuda", generator=g)[:K]].contiguous()
    v0 = torch.full((K, D), 2.0, device="cuda")
    w0 = torch.full((K,), 1.0 / K, dtype=torch.float64, device="cuda")
    gm = S.GaussianMixture(K, D, reg_covar=REG).set_parameters(w0, m0, v0)
    gm.step(x)                                              # (allocates the workspace)
    gm.set_parameters(w0, m0, v0)
    ivar, cst, cdf = gm._ready("gmm_bench")
    lw0 = gm.logw.clone()
    P = MX._partials(K, D, N)
    L, p, st = MX.L, MX._p, MX._st

    def restart():
        gm.logw.copy_(lw0)
        gm.mean.copy_(m0)
        gm.var.copy_(v0)
        L.call("sv_gmm_prepare", p(gm.logw), p(gm.mean), p(gm.var), K, D, p(ivar), p(cst), p(cdf), st())

    def fused():
        restart()
        return gm.step(x)

    tl, tm, tv = lw0.clone(), m0.clone(), v0.clone()

    def torch_way():
        tl.copy_(lw0)
        tm.copy_(m0)
        tv.copy_(v0)
        return torch_step(x, x2, tl, tm, tv)

    stats = fused().clone()
    ours = (gm.logw.clone(), gm.mean.clone(), gm.var.clone())
    theirs = torch_way()
    diff = [float((a.double() - b.double()).abs().max()) for a, b in zip(ours, theirs[:3])]
    bound = abs(float(stats[0]) - float(theirs[3]))

    restart()
    lse, sums, counts, _ = gm._workspace(N, x.device)
    parts = [("sv_gmm_estep", lambda: L.call("sv_gmm_estep", p(x), N, p(ivar), p(gm.mean), p(cst), K, D, p(lse), None, None, st())),
             ("sv_gmm_accum", lambda: L.call("sv_gmm_accum", p(x), p(lse), N, p(ivar), p(gm.mean), p(cst), K, D, p(sums), p(counts), P, 1, st())),
             ("restart + finish", lambda: (restart(), L.call("sv_gmm_finish", p(sums), p(counts), P, K, D, REG, p(gm.logw), p(gm.mean), p(gm.var),
                                                             p(ivar), p(cst), p(cdf), p(gm.stats), st()))),
             ("restart alone", restart)]
    for _, fn in parts[:2]:
        fn()
    runs = [("fused eager", fused), ("fused graph", graphed(fused)), ("torch eager", torch_way), ("torch graph", graphed(torch_way))] + parts
    got = {}
    for name, fn in runs:
        if fn is None:
            continue
        med, lo, hi = timed_ms(fn, WARM, REPS, PASSES)
        got[name] = med
        print("K=%-4d P=%2d  %-17s: %9.4f ms  (min %.4f .. max %.4f; %d x %d passes)" % (K, P, name, med, lo, hi, REPS, PASSES), flush=True)
    for kind in ("eager", "graph"):
        if "fused " + kind in got and "torch " + kind in got:
            print("K=%-4d torch / fused (%s) = %.2f" % (K, kind, got["torch " + kind] / got["fused " + kind]), flush=True)
    print("K=%-4d max |difference| after one iteration: logw %.1e  mean %.1e  var %.1e  bound %.1e" % ((K,) + tuple(diff) + (bound,)), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "tools/gmm_bench.py measures on an MI355X: no GPU here"
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(int(sys.argv[2]))
        sys.exit(0)
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gmm_bench.txt"))
    ap.add_argument("--items", default=",".join(ITEMS))
    a = ap.parse_args()
    lines = ["one EM iteration of a diagonal Gaussian mixture, N = %d, D = %d, fp32, %s (tools/gmm_bench.py)" % (N, D, torch.cuda.get_device_name(0))]
    print(lines[0], flush=True)
    for item in a.items.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", item], timeout=300, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        sys.stderr.write(r.stderr[-2000:])
        lines += r.stdout.splitlines()
        if r.returncode != 0:
            sys.exit("tools/gmm_bench.py: K = %s failed (exit status %d); nothing further was started" % (item, r.returncode))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
