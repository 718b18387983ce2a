"""One exact t-SNE iteration at a fixed shape -- N = 10 000 / 50 000 points, d = 2, k = 90 neighbours, perplexity 30 -- two ways:
  fused   sv_tsne_attract + sv_tsne_repulse + sv_tsne_update (shot_vae_amd.embed.TSNE.step): no [N, N] matrix exists, no float atomic,
          the same bits every time
  torch   torch.cdist, elementwise ops over the [N, N] matrix (w, w^2, Z, the repulsion as a row sum and a matmul), index_add_ for the
          sparse attraction, the gains / momentum update elementwise: stores several [N, N] fp32 temporaries (10 GB each at 50 000),
          float atomics in index_add_
each eager and replayed from a captured graph (torch.cuda.graph), plus the three fused launches timed on their own and the one-off
costs of a fit (LatentIndex.search, sv_tsne_affinity, symmetrize; D = 32).  One size per process: the driver starts a fresh child for
each, one after the other, and stops at the first that fails.  In a child every way runs in the same process state after its own
warm-up (3 passes): the median of 7 timings of 20 back-to-back passes, each timing ending in a device synchronise (tools/
cluster_bench.py's protocol).  The child asserts that the two ways agree on the first step from one state (the velocities within 1 % of
the largest).  No ratio is required: the file records what was measured (profiles/tsne_bench.txt).  Fails without a GPU.
Usage: python tools/tsne_bench.py [--out profiles/tsne_bench.txt] [--items 10000,50000] | --one N"""
import argparse
import os
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shot_vae_amd as S                                   # noqa: E402
from shot_vae_amd import embed as E                        # noqa: E402
from tools.cluster_bench import graphed                    # noqa: E402
from tools.knn_bench import timed_ms                       # noqa: E402

D, DIM, K, PERPLEXITY, CLASSES = 32, 2, 90, 30.0, 10
ITEMS = ("10000", "50000")
WARM, REPS, PASSES = 3, 7, 20


def torch_step(y, vel, gain, rows, cols, vals, attr, e, mom, lr):
    d2 = torch.cdist(y, y).square_()
    w = 1.0 / (1.0 + d2)
    w.fill_diagonal_(0.0)
    Z = w.sum()
    w2 = w * w
    rep = w2.sum(dim=1, keepdim=True) * y - w2 @ y
    diff = y[rows] - y[cols]
    pw = vals / (1.0 + (diff * diff).sum(dim=1))
    attr.zero_().index_add_(0, rows, pw[:, None] * diff)
    g = 4.0 * (e * attr - rep / Z)
    gain.copy_(torch.where(vel * g < 0, gain + 0.2, gain * 0.8).clamp_(min=0.01))
    vel.mul_(mom).sub_(lr * gain * g)
    y.add_(vel)


def once_ms(fn, reps=3):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2], out


def one(N):
    g = torch.Generator(device="cuda").manual_seed(0)
    centres = 3.0 * torch.randn(CLASSES, D, device="cuda", generator=g)
    x = centres[torch.randint(0, CLASSES, (N,), device="cuda", generator=g)] + torch.randn(N, D, device="cuda", generator=g)
    y0 = 10.0 * torch.randn(N, DIM, device="cuda", generator=g)

    # the one-off costs of a fit
    index = S.LatentIndex(D, "euclid")
    index.add(x)
    t_search, (dist, idx) = once_ms(lambda: index.search(x, None, k=K, exclude_self_from=0))
    t_aff, (pc, beta, steps) = once_ms(lambda: S.conditional_affinities(dist, idx, PERPLEXITY))
    t_sym, (rowptr, col, val) = once_ms(lambda: S.symmetrize(pc, idx))
    print("N=%-6d one-off: search %.3f ms, sv_tsne_affinity %.3f ms (at most %d steps), symmetrize %.3f ms (%d entries)"
          % (N, t_search, t_aff, int(steps.max()), t_sym, col.numel()), flush=True)

    ts = S.TSNE(perplexity=PERPLEXITY, k=K, init=y0).prepare(x)
    assert torch.equal(ts.col, col) and torch.equal(ts.val, val)
    rows = torch.repeat_interleave(torch.arange(N, device="cuda"), rowptr[1:] - rowptr[:-1])
    ty, tvel, tgain, tattr = y0.clone(), torch.zeros_like(y0), torch.ones_like(y0), torch.empty_like(y0)
    e, mom, lr = (float(v) for v in ts.hyper.cpu())

    def torch_way():
        torch_step(ty, tvel, tgain, rows, col, val, tattr, e, mom, lr)

    ts.step()
    torch_way()
    err, top = float((ts.vel - tvel).abs().max()), float(ts.vel.abs().max())
    assert err <= 1e-2 * top, "fused and torch disagree on the first step: velocities differ by %g of %g" % (err, top)
    stats = ts.stats.cpu().tolist()

    L, p, st = E.L, E._p, E._st
    parts = [("sv_tsne_attract", lambda: L.call("sv_tsne_attract", p(ts.y), N, DIM, p(ts.rowptr), p(ts.col), p(ts.val), p(ts.attr), p(ts.rowkl),
                                                st())),
             ("sv_tsne_repulse", lambda: L.call("sv_tsne_repulse", p(ts.y), N, DIM, ts.P, p(ts.rep), p(ts.z), st())),
             ("sv_tsne_update", lambda: L.call("sv_tsne_update", p(ts.y), p(ts.vel), p(ts.gain), p(ts.attr), p(ts.rowkl), p(ts.rep), p(ts.z),
                                               ts.P, N, DIM, p(ts.hyper), p(ts.scratch), p(ts.stats), st()))]
    runs = [("fused eager", ts.step), ("fused graph", graphed(ts.step)), ("torch eager", torch_way), ("torch graph", graphed(torch_way))] + parts
    got = {}
    for name, fn in runs:
        if fn is None:
            continue
        med, lo, hi = timed_ms(fn, WARM, REPS, PASSES)
        got[name] = med
        print("N=%-6d P=%2d  %-17s: %9.4f ms  (min %.4f .. max %.4f; %d x %d passes)" % (N, ts.P, name, med, lo, hi, REPS, PASSES), flush=True)
    for kind in ("eager", "graph"):
        if "fused " + kind in got and "torch " + kind in got:
            print("N=%-6d torch / fused (%s) = %.2f" % (N, kind, got["torch " + kind] / got["fused " + kind]), flush=True)
    print("N=%-6d sv_tsne_repulse: %.2f G pairs/s" % (N, N * (N - 1.0) / got["sv_tsne_repulse"] / 1e6), flush=True)
    print("N=%-6d first step: KL %.4f, Z %.6g, |g|^2 %.4g; max |velocity difference| = %.1e of %.1e" % ((N,) + tuple(stats) + (err, top)),
          flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "tools/tsne_bench.py measures on an MI355X: no GPU here"
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(int(sys.argv[2]))
        sys.exit(0)
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tsne_bench.txt"))
    ap.add_argument("--items", default=",".join(ITEMS))
    a = ap.parse_args()
    lines = ["one exact t-SNE iteration, d = %d, k = %d, perplexity %g, fp32, %s (tools/tsne_bench.py)"
             % (DIM, K, PERPLEXITY, torch.cuda.get_device_name(0))]
    print(lines[0], flush=True)
    for item in a.items.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", item], timeout=500, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        sys.stderr.write(r.stderr[-2000:])
        lines += r.stdout.splitlines()
        if r.returncode != 0:
            sys.exit("tools/tsne_bench.py: N = %s failed (exit status %d); nothing further was started" % (item, r.returncode))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
