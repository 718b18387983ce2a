"""Kernel two-sample statistics at fixed shapes, two ways each:
  rbf1 / rbf5 / poly   the weighted row sums sum_j k(x_i, y_j) at Q = 10 000, N = 50 000, D = 128 (fp32 rows): RBF with one scale,
                       RBF with five scales, the cubic polynomial kernel
      fused   shot_vae_amd.twosample.kernel_sums (sv_ksum_scan + sv_ksum_finish): no [Q, N] temporary, double sums in a fixed order
      torch   row chunks of 2 048: cdist ** 2 (or the matmul), the kernel function, sum(dtype=float64) -- a [2048, N] temporary or two
  kid                  kid() at 100 subsets x 1 000 rows x 128 (three batched scans) against a bmm formulation of the same sums
  perm                 permutation_test() at 2 000 pooled rows x 200 permutations (one scan with 201 weight vectors) against the
                       kernel matrix stored once and W K W^T by two matmuls
One item per process: the driver starts a fresh child for each, one after the other, and stops at the first that fails.  In a child
both ways run in the same process state after their own warm-up (2 passes): the median of 7 timings of 5 back-to-back passes, each
timing ending in a device synchronise.  The scan items are set beside sv_ball_scan (profiles/quality_bench.txt) and sv_aggpost_scan
(profiles/aggpost_bench.txt) at the same shape.  No ratio is required: the file records what was measured
(profiles/twosample_bench.txt).  Fails without a GPU.
Usage: python tools/twosample_bench.py [--out profiles/twosample_bench.txt] [--items rbf1,rbf5,poly,kid,perm] | --one ITEM"""
import argparse
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shot_vae_amd import twosample as TS                   # noqa: E402
from tools.knn_bench import timed_ms                       # noqa: E402

Q, N, D = 10000, 50000, 128
CHUNK = 2048
ITEMS = ("rbf1", "rbf5", "poly", "kid", "perm")
WARM, REPS, PASSES = 2, 7, 5
BALL_MS, AGGPOST_MS = 4.366, 7.552      # profiles/quality_bench.txt, profiles/aggpost_bench.txt: the sibling scans at Q x N x D
LADDER = (0.25, 0.5, 1.0, 2.0, 4.0)


def rows(n, seed, shift=0.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(n, D, device="cuda", generator=g) + shift).contiguous()


def report(item, ways, unit="ms"):
    got = {}
    for name, fn in ways:
        med, lo, hi = timed_ms(fn, WARM, REPS, PASSES)
        got[name] = med
        print("%-5s %-6s: %10.3f %s  (min %.3f .. max %.3f; %d x %d passes)" % (item, name, med, unit, lo, hi, REPS, PASSES), flush=True)
    print("%-5s torch / fused = %.2f" % (item, got["torch"] / got["fused"]), flush=True)
    return got


def scan_item(item):
    x, y = rows(Q, 1), rows(N, 2, 0.1)
    a = TS.median_bandwidth(x, y)                                  # a device scalar: no host read in the timed calls
    if item == "poly":
        kernel, gamma, kp = "poly", None, None
    else:
        kernel = "rbf"
        gamma = a.reshape(1) if item == "rbf1" else a * torch.tensor(LADDER, dtype=torch.float64, device="cuda")
        kp = TS.kernel_params("rbf", gamma, D, x.device)

    def fused():
        return TS.kernel_sums(x, y, kernel, gamma)

    def torch_way():
        out = torch.empty(Q, dtype=torch.float64, device="cuda")
        for i in range(0, Q, CHUNK):
            xc = x[i:i + CHUNK]
            if kernel == "poly":
                k = (xc @ y.t() / D + 1.0) ** 3
            else:
                d = torch.cdist(xc, y) ** 2
                k = sum(float(1.0 / kp.shape[0]) * torch.exp(-kp[s, 0].float() * d) for s in range(kp.shape[0]))
            out[i:i + CHUNK] = k.sum(dim=1, dtype=torch.float64)
        return out

    ours, theirs = fused(), torch_way()
    rel = float(((ours - theirs).abs() / theirs.abs()).max())
    print("%-5s Q = %d, N = %d, D = %d; torch holds a [%d, %d] fp32 temporary (%.0f MB) per intermediate; the whole matrix would be %.1f GB" % (
        item, Q, N, D, CHUNK, N, 4e-6 * CHUNK * N, 4e-9 * Q * N), flush=True)
    got = report(item, (("fused", fused), ("torch", torch_way)))
    print("%-5s fused / sv_ball_scan (%.3f ms) = %.2f, fused / sv_aggpost_scan (%.3f ms) = %.2f at the same shape" % (
        item, BALL_MS, got["fused"] / BALL_MS, AGGPOST_MS, got["fused"] / AGGPOST_MS), flush=True)
    print("%-5s largest relative difference of a row sum, fused (fp32 pairs, double function and sums) against torch (fp32): %.1e" % (item, rel),
          flush=True)
    again = fused()
    print("%-5s a repeated fused call gives the same bits: %s" % (item, bool(torch.equal(ours, again))), flush=True)


def kid_item():
    subsets, size = 100, 1000
    real, fake = rows(20000, 3), rows(20000, 4, 0.05)

    ia, ib = (t.cuda() for t in TS.subset_indices(real.shape[0], fake.shape[0], subsets, size, 0))
    kparam = TS.kernel_params("poly", None, D, real.device)

    def fused():                                                   # kid() behind its index sets: the gathers, three batched scans
        vals = TS._mmd2_of(TS.L.KSUM_POLY, kparam, 3, real[ia].contiguous(), fake[ib].contiguous(), True)
        return torch.stack([vals.mean(), vals.std(unbiased=False)])

    def torch_way():
        xs, ys = real[ia], fake[ib]                                # [subsets, size, D]
        kxx = (torch.bmm(xs, xs.transpose(1, 2)) / D + 1.0) ** 3
        kyy = (torch.bmm(ys, ys.transpose(1, 2)) / D + 1.0) ** 3
        kxy = (torch.bmm(xs, ys.transpose(1, 2)) / D + 1.0) ** 3
        sxx = kxx.sum(dim=(1, 2), dtype=torch.float64) - torch.diagonal(kxx, dim1=1, dim2=2).sum(dim=1, dtype=torch.float64)
        syy = kyy.sum(dim=(1, 2), dtype=torch.float64) - torch.diagonal(kyy, dim1=1, dim2=2).sum(dim=1, dtype=torch.float64)
        vals = sxx / (size * (size - 1)) + syy / (size * (size - 1)) - 2.0 * kxy.sum(dim=(1, 2), dtype=torch.float64) / (size * size)
        return torch.stack([vals.mean(), vals.std(unbiased=False)])

    ours, theirs = fused(), torch_way()
    print("kid   %d subsets x %d rows x %d (the index sets are drawn on the host before the timed calls; both ways gather); torch holds "
          "three [%d, %d, %d] fp32 matrices (%.1f GB)" % (subsets, size, D, subsets, size, size, 3 * 4e-9 * subsets * size * size), flush=True)
    report("kid", (("fused", fused), ("torch", torch_way)))
    print("kid   mean %.6e (fused) %.6e (torch); std %.6e (fused) %.6e (torch)" % (float(ours[0]), float(theirs[0]), float(ours[1]), float(theirs[1])),
          flush=True)


def perm_item():
    n = m = 1000
    B = 200
    x, y = rows(n, 5), rows(m, 6, 0.05)
    a = TS.median_bandwidth(x, y)
    gen = torch.Generator().manual_seed(0)
    member = torch.zeros(B, n + m, dtype=torch.bool)
    for b in range(B):
        member[b, torch.randperm(n + m, generator=gen)[:n]] = True
    signs = member.cuda()

    def fused():
        return TS._permutation_stats("permutation_test", x, y, "rbf", a, 3, 1.0, None, B, 0, signs)

    first = torch.arange(n + m, device="cuda") < n
    w = TS.split_weights(torch.cat([first[None, :], signs]), n, m).double()
    z = torch.cat([x, y])

    def torch_way():
        k = torch.exp(-a * (torch.cdist(z, z) ** 2).double())     # the matrix is stored once: 32 MB in double
        return ((w @ k) * w).sum(dim=1) / (float(n) * float(m)) ** 2

    ours, theirs = fused(), torch_way()
    print("perm  %d pooled rows x %d permutations x %d; fused: ONE scan with %d weight vectors over shared rows (every problem evaluates "
          "the kernel again); torch: the kernel matrix once, then two matmuls in double" % (n + m, B, D, B + 1), flush=True)
    report("perm", (("fused", fused), ("torch", torch_way)))
    print("perm  largest difference of a statistic: %.1e (observed statistic %.6e)" % (float((ours - theirs).abs().max()), float(ours[0])), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "tools/twosample_bench.py measures on an MI355X: no GPU here"
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        item = sys.argv[2]
        {"kid": kid_item, "perm": perm_item}.get(item, lambda: scan_item(item))()
        sys.exit(0)
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "twosample_bench.txt"))
    ap.add_argument("--items", default=",".join(ITEMS))
    a = ap.parse_args()
    lines = ["kernel two-sample statistics, fp32 rows, double sums, %s (tools/twosample_bench.py)" % torch.cuda.get_device_name(0)]
    print(lines[0], flush=True)
    for item in a.items.split(","):
        if item not in ITEMS:
            sys.exit("tools/twosample_bench.py: unknown item %r" % item)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", item], timeout=280, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        sys.stderr.write(r.stderr[-2000:])
        lines += r.stdout.splitlines()
        if r.returncode != 0:
            sys.exit("tools/twosample_bench.py: %s failed (exit status %d); nothing further was started" % (item, r.returncode))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
