"""k-nearest-neighbour search in latent space at a fixed shape -- Q = 10 000 queries, N = 50 000 gallery rows, D = 128 -- for
k in {1, 20, 200} and the four metrics, three ways:
  search          LatentIndex.search: sv_knn_scan, the distance tiles merged into the k-lists on the chip
  pairdist+topk   sv_pairdist into a [Q, N] fp32 matrix (2 GB), then torch.topk
  torch+topk      the reference's broadcast expression (lib/utils/calculate_dist.py) over chunks of CHUNK query rows -- each of its
                  [chunk, N, D] intermediates is 1.6 GB at CHUNK = 64 -- written into the same matrix, then torch.topk; the cosine
                  is the reference's torch.mm form and needs no chunks
One item (metric, k) per process: the driver starts a fresh child for each, one after the other, and stops at the first that fails.
In a child all three run in the same process state, each after its own warm-up: search and pairdist+topk 3 warm-up passes and the
median of 7 timings of 5 back-to-back passes, torch+topk 1 warm-up pass and the median of 3 single passes (a pass takes seconds).
Every timing ends in a device synchronise.  The child asserts that search returns exactly the values of pairdist+topk (the two
kernels give the same bits per pair; torch.topk breaks ties in its own order, so indices are not compared).  There is no target: the
figures are a record (profiles/knn_bench.txt), with one bar -- search must not be slower than pairdist+topk at k = 20.  Fails without
a GPU.
Usage: python tools/knn_bench.py [--out profiles/knn_bench.txt] [--metrics kl,w2,euclid,cosine] [--ks 1,20,200] | --one METRIC K"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shot_vae_amd as S                                   # noqa: E402

Q, N, D, CHUNK = 10000, 50000, 128, 64
METRICS, KS = ("kl", "w2", "euclid", "cosine"), (1, 20, 200)


def timed_ms(call, warm, reps, n):
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(n):
            call()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / n * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def torch_matrix(metric, u1, l1, u2, l2, out):
    """the reference's expressions, chunked over the query rows"""
    if metric == "cosine":
        n1, n2 = torch.sum(u1 ** 2, dim=1), torch.sum(u2 ** 2, dim=1)
        out.copy_(torch.mm(u1, u2.t()) / (n1.view(-1, 1) * n2.view(1, -1)))
        return out
    v2 = torch.exp(l2) ** 2
    for a in range(0, u1.shape[0], CHUNK):
        q, ql = u1[a:a + CHUNK], l1[a:a + CHUNK]
        if metric == "kl":
            s_pairwise = torch.unsqueeze(torch.exp(ql) ** 2, 1) / torch.unsqueeze(v2, 0)
            u_pairwise = (torch.unsqueeze(q, 1) - torch.unsqueeze(u2, 0)) ** 2 / torch.unsqueeze(v2, 0)
            out[a:a + CHUNK] = 0.5 * (-1 * torch.sum(torch.log(s_pairwise), dim=2) + torch.sum(s_pairwise, dim=2)
                                      + torch.sum(u_pairwise, dim=2) - D)
        else:
            d = torch.sum((q.unsqueeze(1) - u2.unsqueeze(0)) ** 2, dim=2)
            if metric == "w2":
                d = d + torch.sum((torch.exp(ql).unsqueeze(1) - torch.exp(l2).unsqueeze(0)) ** 2, dim=2)
            out[a:a + CHUNK] = d
    return out


def one(metric, k):
    g = torch.Generator(device="cuda").manual_seed(0)
    u1, u2 = torch.randn(Q, D, device="cuda", generator=g), torch.randn(N, D, device="cuda", generator=g)
    l1, l2 = (torch.rand(n, D, device="cuda", generator=g) * 1.5 - 1.0 for n in (Q, N))
    index = S.LatentIndex(D, metric=metric)
    index.add(u2, l2)
    mat = torch.empty(Q, N, dtype=torch.float32, device="cuda")
    largest = metric == "cosine"

    def search():
        return index.search(u1, l1, k)

    def pair():
        S.neighbors.L.call("sv_pairdist", index.code, S.neighbors._p(u1), S.neighbors._p(l1 if index.ls is not None else None), Q,
                           S.neighbors._p(index.mu), S.neighbors._p(index.ls), N, D, S.neighbors._p(mat), N, S.neighbors._st())
        return torch.topk(mat, k, dim=1, largest=largest, sorted=True)

    def ref():
        return torch.topk(torch_matrix(metric, u1, l1, u2, l2, mat), k, dim=1, largest=largest, sorted=True)

    assert torch.equal(search()[0], pair()[0]), "search and pairdist+topk disagree"
    rows = []
    for name, call, warm, reps, n in (("search", search, 3, 7, 5), ("pairdist+topk", pair, 3, 7, 5), ("torch+topk", ref, 1, 3, 1)):
        med, lo, hi = timed_ms(call, warm, reps, n)
        rows.append(med)
        print("%-6s k=%3d  %-13s: %10.3f ms  (min %.3f .. max %.3f; %d x %d passes)" % (metric, k, name, med, lo, hi, reps, n), flush=True)
    print("%-6s k=%3d  pairdist+topk / search = %.2f   torch+topk / search = %.2f" % (metric, k, rows[1] / rows[0], rows[2] / rows[0]), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "tools/knn_bench.py measures on an MI355X: no GPU here"
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(sys.argv[2], int(sys.argv[3]))
        sys.exit(0)
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "knn_bench.txt"))
    ap.add_argument("--metrics", default=",".join(METRICS))
    ap.add_argument("--ks", default=",".join(str(k) for k in KS))
    a = ap.parse_args()
    lines = ["k-NN search, Q = %d, N = %d, D = %d, fp32, %s (tools/knn_bench.py)" % (Q, N, D, torch.cuda.get_device_name(0))]
    print(lines[0], flush=True)
    slower = []
    for metric in a.metrics.split(","):
        for k in (int(v) for v in a.ks.split(",")):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", metric, str(k)], timeout=600, capture_output=True, text=True)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            sys.stderr.write(r.stderr[-2000:])
            lines += r.stdout.splitlines()
            if r.returncode != 0:
                sys.exit("tools/knn_bench.py: %s k=%d failed (exit status %d); nothing further was started" % (metric, k, r.returncode))
            ratio = float(re.search(r"pairdist\+topk / search = ([0-9.]+)", r.stdout).group(1))
            if k == 20 and ratio < 1.0:
                slower.append(metric)
    lines.append("the bar (search not slower than pairdist+topk at k = 20): %s" % ("MISSED for " + ", ".join(slower) if slower else "met"))
    print(lines[-1])
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
