"""One Lloyd iteration of k-means at a fixed shape -- N = 50 000 rows, D = 128, K = 10 / 100 / 1000 centroids -- two ways:
  fused   sv_kmeans_assign + sv_kmeans_accum + sv_kmeans_finish (shot_vae_amd.cluster.KMeans): no [N, K] matrix exists, no float atomic,
          the same bits every time
  torch   torch.cdist + argmin + index_add_ (sums and counts) + the division: stores the [N, K] matrix, float atomics in index_add_
each eager and replayed from a captured graph (torch.cuda.graph), plus the three fused launches timed on their own (what bounds ours).
One item (a K) per process: the driver starts a fresh child for each, one after the other, and stops at the first that fails.  In a
child every way runs in the same process state after its own warm-up (3 passes): the median of 7 timings of 20 back-to-back passes, each
timing ending in a device synchronise.  The child asserts that the two ways agree: the same assignment on >= 99.9 % of the rows (fp32
cdist expands |a|^2 + |b|^2 - 2 a.b and may break a near-tie the other way) and centroids within 1e-3.  No ratio is required: the
file records what was measured (profiles/cluster_bench.txt).  Fails without a GPU.
Usage: python tools/cluster_bench.py [--out profiles/cluster_bench.txt] [--items 10,100,1000] | --one K"""
import argparse
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shot_vae_amd as S                                   # noqa: E402
from shot_vae_amd import cluster as CL                     # noqa: E402
from tools.knn_bench import timed_ms                       # noqa: E402

N, D = 50000, 128
ITEMS = ("10", "100", "1000")
WARM, REPS, PASSES = 3, 7, 20


def torch_step(x, c, sums, counts, ones):
    a = torch.cdist(x, c).argmin(dim=1)
    sums.zero_().index_add_(0, a, x)
    counts.zero_().index_add_(0, a, ones)
    return a, torch.where(counts[:, None] > 0, sums / counts.clamp(min=1.0)[:, None], c)


def graphed(fn):
    """fn captured once (after a warm-up on a side stream) -> a callable that replays it; None when the capture fails"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(graph):
            fn()
    except RuntimeError as e:
        print("     (not capturable: %s)" % str(e).splitlines()[0][:100], flush=True)
        return None
    return graph.replay


def one(K):
    g = torch.Generator(device="cuda").manual_seed(0)
    centres = 3.0 * torch.randn(K, D, device="cuda", generator=g)
    x = centres[torch.randint(0, K, (N,), device="cuda", generator=g)] + torch.randn(N, D, device="cuda", generator=g)
    c = x[torch.randperm(N, device="cuda", generator=g)[:K]].contiguous()
    km = S.KMeans(K, D, init=c).reset()
    out = torch.empty_like(c)
    P = CL._partials(K, D, N)
    sums, counts, ones = torch.empty(K, D, device="cuda"), torch.empty(K, device="cuda"), torch.ones(N, device="cuda")

    def fused():
        return km._lloyd(x, c, out)

    def torch_way():
        return torch_step(x, c, sums, counts, ones)

    fused()
    a_ref, c_ref = torch_way()
    a = km.predict(x)
    same = float((a == a_ref).double().mean())
    err = float((out - c_ref).abs().max())
    assert same >= 0.999 and err <= 1e-3, "fused and torch disagree: %.5f of the rows agree, centroids differ by %g" % (same, err)

    # the three launches on their own
    L, p, st = CL.L, CL._p, CL._st
    assign, dist = CL._assign(x, c)
    s = torch.empty(P, K, D, dtype=torch.float64, device="cuda")
    n = torch.empty(P, K, dtype=torch.int64, device="cuda")
    i = torch.empty(P, dtype=torch.float64, device="cuda")
    cnt, stats = torch.empty(K, dtype=torch.int64, device="cuda"), torch.empty(2, device="cuda")
    parts = [("sv_kmeans_assign", lambda: L.call("sv_kmeans_assign", p(x), N, p(c), K, D, p(assign), p(dist), st())),
             ("sv_kmeans_accum", lambda: L.call("sv_kmeans_accum", p(x), p(assign), p(dist), N, D, K, p(s), p(n), p(i), P, 1, st())),
             ("sv_kmeans_finish", lambda: L.call("sv_kmeans_finish", p(s), p(n), p(i), P, K, D, p(c), p(out), p(cnt), p(stats), st()))]
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
    print("K=%-4d rows assigned alike = %.5f   max |centroid difference| = %.1e" % (K, same, err), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "tools/cluster_bench.py measures on an MI355X: no GPU here"
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(int(sys.argv[2]))
        sys.exit(0)
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cluster_bench.txt"))
    ap.add_argument("--items", default=",".join(ITEMS))
    a = ap.parse_args()
    lines = ["one Lloyd iteration of k-means, N = %d, D = %d, fp32, %s (tools/cluster_bench.py)" % (N, D, torch.cuda.get_device_name(0))]
    print(lines[0], flush=True)
    for item in a.items.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", item], timeout=300, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        sys.stderr.write(r.stderr[-2000:])
        lines += r.stdout.splitlines()
        if r.returncode != 0:
            sys.exit("tools/cluster_bench.py: K = %s failed (exit status %d); nothing further was started" % (item, r.returncode))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
