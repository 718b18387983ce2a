"""One iteration of label spreading at a fixed shape -- N = 50 000 rows, k = 7 / 30 neighbours, K = 10 / 100 classes, the symmetrised
k-NN graph of 32-dimensional blobs (shot_vae_amd.knn_graph, "euclid") -- two ways:
  fused   sv_lp_step (shot_vae_amd.propagate.LabelPropagator.step): the gather, the clamp and the statistics in one launch plus a
          one-block merge; double accumulation in segment order, no atomic, the same bits every time
  torch   alpha * torch.sparse.mm(S, F) + (1 - alpha) Y on the SAME CSR matrix, then (F_new - F).abs().sum(): fp32 sums in whatever
          order the sparse library takes
each eager and replayed from a captured graph (torch.cuda.graph), plus the fused gather without its statistics (what they cost).  A pass is TWO iterations (the buffers change roles, so a captured
graph holds an even number of steps); the times printed are per iteration.  One item (a shape) per process: the driver starts a fresh
child for each, one after the other, and stops at the first that fails.  In a child every way runs in the same process state after its
own warm-up (3 passes): the median of 7 timings of 20 back-to-back passes, each timing ending in a device synchronise.  Beside the times
the child prints the traffic floor of an iteration -- nnz (12 + 4 K) + 8 N K bytes: every entry's column, weight and gathered row of K
floats once, F read once for the statistics and written once -- and the rate the fused time amounts to.  No ratio is required: the file
records what was measured (profiles/labelprop_bench.txt).  Fails without a GPU.
Usage: python tools/labelprop_bench.py [--out profiles/labelprop_bench.txt] [--items 7x10,30x10,7x100,30x100] | --one kxK"""
import argparse
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shot_vae_amd as S                                   # noqa: E402
from shot_vae_amd import propagate as PG                   # noqa: E402
from tools.cluster_bench import graphed                    # noqa: E402
from tools.knn_bench import timed_ms                       # noqa: E402

N, DIM = 50000, 32
ITEMS = ("7x10", "30x10", "7x100", "30x100")
WARM, REPS, PASSES = 3, 7, 20
ALPHA = 0.2


def one(k, K):
    g = torch.Generator(device="cuda").manual_seed(0)
    centres = 1.2 * torch.randn(K, DIM, device="cuda", generator=g)
    cls = torch.randint(0, K, (N,), device="cuda", generator=g)
    x = (centres[cls] + torch.randn(N, DIM, device="cuda", generator=g)).contiguous()
    y = S.select_labels(cls, 10, K, seed=0)
    rowptr, col, val = S.knn_graph(x, None, k=k, metric="euclid")
    lp = S.LabelPropagator(K, "spreading", alpha=ALPHA).prepare_graph(rowptr, col, val, y)
    nnz = lp.nnz
    degree = rowptr[1:] - rowptr[:-1]

    def fused():
        lp.step()
        return lp.step()

    def gather_alone():
        # the same two iterations without the statistics: no |F_new - F| pass, no merge launch
        for a, b in ((0, 1), (1, 0)):
            PG.L.call("sv_lp_step", PG._p(lp.f[a]), N, PG._p(lp.rowptr), PG._p(lp.col), PG._p(lp.sval), nnz, N, K, PG._p(lp.label), PG.L.LP_SPREADING,
                      ALPHA, 1.0 - ALPHA, PG._p(lp.f[b]), None, None, PG._st())

    sp = torch.sparse_csr_tensor(rowptr, col, lp.sval, size=(N, N))
    static = (1.0 - ALPHA) * lp.f[0].clone()
    bufs = [lp.f[0].clone(), torch.empty_like(lp.f[0])]

    def torch_way():
        delta = None
        for a, b in ((0, 1), (1, 0)):
            torch.add(static, torch.sparse.mm(sp, bufs[a]), alpha=ALPHA, out=bufs[b])
            delta = (bufs[b] - bufs[a]).abs().sum()
        return delta

    lp.reset()
    ours = fused().clone()
    theirs = torch_way()
    diff, ours, theirs = float((lp.f[lp.cur] - bufs[0]).abs().max()), float(ours[0]), float(theirs)

    floor = nnz * (12 + 4 * K) + 8 * N * K
    print("k=%-3d K=%-4d nnz %d (degree %d .. %d), F %.1f MB, traffic floor %.2f MB per iteration" % (k, K, nnz, int(degree.min()), int(degree.max()),
                                                                                                   4e-6 * N * K, 1e-6 * floor), flush=True)
    got = {}
    # (the capture of the torch way comes last, and nothing touches the device after it: where the sparse product cannot be captured, the
    # failed capture leaves the stream in error)
    for name, make in (("fused eager", lambda: fused), ("fused graph", lambda: graphed(fused)), ("gather alone", lambda: gather_alone),
                       ("torch eager", lambda: torch_way),
                       ("torch graph", lambda: graphed(torch_way))):
        fn = make()
        if fn is None:
            continue
        med, lo, hi = timed_ms(fn, WARM, REPS, PASSES)
        got[name] = med / 2
        print("k=%-3d K=%-4d %-12s: %9.4f ms per iteration  (min %.4f .. max %.4f; %d x %d passes of 2)" % (k, K, name, med / 2, lo / 2, hi / 2, REPS, PASSES),
              flush=True)
    for kind in ("eager", "graph"):
        if "fused " + kind in got and "torch " + kind in got:
            print("k=%-3d K=%-4d torch / fused (%s) = %.2f" % (k, K, kind, got["torch " + kind] / got["fused " + kind]), flush=True)
    best = min(v for n, v in got.items() if n.startswith("fused"))
    print("k=%-3d K=%-4d the floor over the fused time: %.0f GB/s" % (k, K, 1e-9 * floor / (1e-3 * best)), flush=True)
    print("k=%-3d K=%-4d after two iterations: max |F difference| %.1e, delta_l1 %.6e (fused) %.6e (torch)" % (k, K, diff, ours, theirs),
          flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "tools/labelprop_bench.py measures on an MI355X: no GPU here"
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(*(int(v) for v in sys.argv[2].split("x")))
        sys.exit(0)
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "labelprop_bench.txt"))
    ap.add_argument("--items", default=",".join(ITEMS))
    a = ap.parse_args()
    lines = ["one iteration of label spreading, N = %d, fp32 storage, double accumulation, %s (tools/labelprop_bench.py)" % (N, torch.cuda.get_device_name(0))]
    print(lines[0], flush=True)
    for item in a.items.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", item], timeout=300, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        sys.stderr.write(r.stderr[-2000:])
        lines += r.stdout.splitlines()
        if r.returncode != 0:
            sys.exit("tools/labelprop_bench.py: %s failed (exit status %d); nothing further was started" % (item, r.returncode))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
