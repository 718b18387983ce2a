"""One iteration of the linear probe's solver at a fixed shape -- N = 50 000 rows, (D, K) = (128, 10) / (640, 100) -- two ways:
  fused   sv_probe_rows + sv_probe_accum + sv_probe_update (shot_vae_amd.probe.LinearProbe.step): no [N, K] matrix exists, no atomic,
          the same bits every time, the step in double
  torch   x @ W^T + b, log_softmax, (p - onehot)^T @ x and the same Nesterov update in fp32: stores the [N, K] matrix
each eager and replayed from a captured graph (torch.cuda.graph), plus the three fused launches timed on their own (what bounds ours).
One item (a shape) per process: the driver starts a fresh child for each, one after the other, and stops at the first that fails.  In a
child every way starts every pass from the SAME point (a copy back, inside the timed region of both ways) and runs in the same process
state after its own warm-up (3 passes): the median of 7 timings of 20 back-to-back passes, each timing ending in a device synchronise.
The child prints the largest difference between the two look-ahead points after one iteration.  No ratio is required: the file records
what was measured (profiles/probe_bench.txt).  Fails without a GPU.
Usage: python tools/probe_bench.py [--out profiles/probe_bench.txt] [--items 128x10,640x100] | --one DxK"""
import argparse
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shot_vae_amd as S                                   # noqa: E402
from shot_vae_amd import probe as PB                       # noqa: E402
from tools.cluster_bench import graphed                    # noqa: E402
from tools.knn_bench import timed_ms                       # noqa: E402

N = 50000
ITEMS = ("128x10", "640x100")
WARM, REPS, PASSES = 3, 7, 20
LAM, LIP, BETA = 1.0 / N, 0.9, 0.95


def torch_step(x, hot, w, b, tw, tb):
    """(w, b): the look-ahead point, (tw, tb): the iterate; all updated in place -> the objective at the old look-ahead point"""
    logp = torch.log_softmax(torch.addmm(b, x, w.t()), dim=1)
    r = logp.exp() - hot
    gw = (r.t() @ x) / N + LAM * w
    gb = r.sum(dim=0) / N
    obj = -(logp * hot).sum() / N + 0.5 * LAM * (w * w).sum()
    nw, nb = w - gw / LIP, b - gb / LIP
    w.copy_(nw + BETA * (nw - tw))
    b.copy_(nb + BETA * (nb - tb))
    tw.copy_(nw)
    tb.copy_(nb)
    return obj


def one(D, K):
    g = torch.Generator(device="cuda").manual_seed(0)
    centres = torch.randn(K, D, device="cuda", generator=g)
    y = torch.randint(0, K, (N,), device="cuda", generator=g)
    x = (centres[y] + torch.randn(N, D, device="cuda", generator=g)).contiguous()
    hot = torch.nn.functional.one_hot(y, K).float()
    start = 0.05 * torch.randn(K, D + 1, device="cuda", generator=g, dtype=torch.float64)
    lp = S.LinearProbe(K, D, standardize=False).start(x.device, LAM, LIP, BETA)
    lp.step(x, y)                                           # (allocates the workspace)
    P = PB._partials(K, D, N)
    L, p, st = PB.L, PB._p, PB._st

    def restart():
        lp.theta.copy_(start)
        lp.look.copy_(start)
        lp.w.copy_(start[:, 1:])
        lp.b.copy_(start[:, 0])

    def fused():
        restart()
        return lp.step(x, y)

    w, b, tw, tb = (torch.empty(K, D, device="cuda"), torch.empty(K, device="cuda"), torch.empty(K, D, device="cuda"), torch.empty(K, device="cuda"))

    def torch_way():
        for t in (w, tw):
            t.copy_(start[:, 1:])
        for t in (b, tb):
            t.copy_(start[:, 0])
        return torch_step(x, hot, w, b, tw, tb)

    stats = fused().clone()
    theirs = torch_way()
    diff = (float((lp.look[:, 1:] - w.double()).abs().max()), float((lp.look[:, 0] - b.double()).abs().max()), abs(float(stats[0]) - float(theirs)))

    restart()
    lse, loss, sums, counts, _ = lp._workspace(N, x.device)
    parts = [("sv_probe_rows", lambda: L.call("sv_probe_rows", p(x), N, p(lp.w), p(lp.b), K, D, p(y), p(lse), p(loss), None, None, st())),
             ("sv_probe_accum", lambda: L.call("sv_probe_accum", p(x), p(y), p(lse), p(loss), N, p(lp.w), p(lp.b), K, D, p(sums), p(counts), P, 1,
                                               None, st())),
             # (the update consumes the states: on a repeat it merges what the last one left, at the same cost)
             ("restart + update", lambda: (restart(), L.call("sv_probe_update", p(sums), p(counts), P, K, D, LAM, 1.0 / LIP, BETA, p(lp.theta),
                                                             p(lp.look), p(lp.w), p(lp.b), p(lp.stats), st()))),
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
        print("D=%-4d K=%-4d P=%2d  %-18s: %9.4f ms  (min %.4f .. max %.4f; %d x %d passes)" % (D, K, P, name, med, lo, hi, REPS, PASSES), flush=True)
    for kind in ("eager", "graph"):
        if "fused " + kind in got and "torch " + kind in got:
            print("D=%-4d K=%-4d torch / fused (%s) = %.2f" % (D, K, kind, got["torch " + kind] / got["fused " + kind]), flush=True)
    print("D=%-4d K=%-4d max |difference| after one iteration: weights %.1e  intercepts %.1e  objective %.1e" % ((D, K) + diff), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "tools/probe_bench.py measures on an MI355X: no GPU here"
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(*(int(v) for v in sys.argv[2].split("x")))
        sys.exit(0)
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "probe_bench.txt"))
    ap.add_argument("--items", default=",".join(ITEMS))
    a = ap.parse_args()
    lines = ["one iteration of the linear probe's solver, N = %d, fp32 scans, double step, %s (tools/probe_bench.py)" % (N, torch.cuda.get_device_name(0))]
    print(lines[0], flush=True)
    for item in a.items.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", item], timeout=300, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        sys.stderr.write(r.stderr[-2000:])
        lines += r.stdout.splitlines()
        if r.returncode != 0:
            sys.exit("tools/probe_bench.py: %s failed (exit status %d); nothing further was started" % (item, r.returncode))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
