"""The silhouette of every row at fixed shapes: n = 10 000 and 50 000 rows x 128 (fp32), K = 10 / 100 / 1000 clusters of random size,
four ways each:
  eager    shot_vae_amd.validity.silhouette_samples: the stable sort, the gather, sv_sil_scan + sv_sil_finish, the scatter back
  replay   the two raw launches (silhouette_grouped on rows grouped beforehand) replayed from a captured graph
  torch    (a) row chunks of 2 048: cdist, a matmul with the one-hot matrix [n, K], the epilogue (gather, divide, masked min, s) in
           torch -- a [2048, n] temporary per chunk
  ksum     (b) sv_ksum_scan + sv_ksum_finish (IMQ, one scale) at the same Q x N x D: the same tile and the same loads with every tile
           full -- the ceiling of this tile design
One item per process: the driver starts a fresh child for each, one after the other, and stops at the first that fails.  In a child
all ways run in the same process state after their own warm-up (2 passes): the median of 5 timings of 3 back-to-back passes, each
timing ending in a device synchronise.  No ratio is required: the file records what was measured (profiles/validity_bench.txt).
Fails without a GPU.
Usage: python tools/validity_bench.py [--out profiles/validity_bench.txt] [--items 10000x10,...] | --one NxK"""
import argparse
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shot_vae_amd import twosample as TS                   # noqa: E402
from shot_vae_amd import validity as V                     # noqa: E402
from tools.knn_bench import timed_ms                       # noqa: E402

D = 128
CHUNK = 2048
ITEMS = tuple("%dx%d" % (n, k) for n in (10000, 50000) for k in (10, 100, 1000))
WARM, REPS, PASSES = 2, 5, 3


def one(item):
    n, K = (int(v) for v in item.split("x"))
    g = torch.Generator(device="cuda").manual_seed(n + K)
    lab = torch.randint(0, K, (n,), device="cuda", generator=g)
    centers = 3.0 * torch.randn(K, D, device="cuda", generator=g)
    x = (torch.randn(n, D, device="cuda", generator=g) + centers[lab]).contiguous()

    def eager():
        return V.silhouette_samples(x, lab, K)

    key, order, seg = V._group("validity_bench", x, lab, K)
    rows, skey = x.index_select(0, order).contiguous(), key.index_select(0, order).contiguous()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        V.silhouette_grouped(rows, skey, rows, seg, K)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = V.silhouette_grouped(rows, skey, rows, seg, K)

    def replay():
        graph.replay()
        return captured[0]

    def torch_way():
        onehot = torch.nn.functional.one_hot(lab, K).float()
        counts = onehot.sum(dim=0)
        out = torch.empty(n, dtype=torch.float32, device="cuda")
        for i in range(0, n, CHUNK):
            lc = lab[i:i + CHUNK, None]
            sums = torch.cdist(x[i:i + CHUNK], x) @ onehot
            own_n = counts[lc[:, 0]]
            a = sums.gather(1, lc)[:, 0] / (own_n - 1.0).clamp(min=1.0)
            means = (sums / counts[None, :].clamp(min=1.0)).masked_fill(counts[None, :] == 0.0, float("inf"))
            b = means.scatter_(1, lc, float("inf")).min(dim=1).values
            s = (b - a) / torch.maximum(a, b)
            out[i:i + CHUNK] = torch.where(own_n > 1.0, s, torch.zeros_like(s))
        return out

    def ksum():
        return TS.kernel_sums(x, x, "imq", 1.0)

    ours, theirs = eager(), torch_way()
    sizes = (seg[1:] - seg[:-1])
    print("%-10s n = %d, K = %d, D = %d; cluster sizes %d .. %d; P = %d; torch holds a [%d, %d] fp32 temporary (%.0f MB) per chunk; the "
          "whole matrix would be %.1f GB" % (item, n, K, D, int(sizes.min()), int(sizes.max()), V.default_partials(n, n, K), CHUNK, n,
                                           4e-6 * CHUNK * n, 4e-9 * n * n), flush=True)
    got = {}
    for name, fn in (("eager", eager), ("replay", replay), ("torch", torch_way), ("ksum", ksum)):
        med, lo, hi = timed_ms(fn, WARM, REPS, PASSES)
        got[name] = med
        print("%-10s %-6s: %10.3f ms  (min %.3f .. max %.3f; %d x %d passes)" % (item, name, med, lo, hi, REPS, PASSES), flush=True)
    print("%-10s torch / eager = %.2f, torch / replay = %.2f, replay / ksum = %.2f; pairs per second of the replay: %.2e" % (
        item, got["torch"] / got["eager"], got["torch"] / got["replay"], got["replay"] / got["ksum"], n * float(n) / (1e-3 * got["replay"])),
        flush=True)
    print("%-10s mean silhouette %.6f (fused) %.6f (torch); largest difference of a row: %.1e" % (
        item, float(ours.mean()), float(theirs.double().mean()), float((ours - theirs.double()).abs().max())), flush=True)
    print("%-10s a repeated eager call gives the same bits: %s; the replay equals it: %s" % (
        item, bool(torch.equal(ours, eager())), bool(torch.equal(replay(), ours.index_select(0, order)))), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "tools/validity_bench.py measures on an MI355X: no GPU here"
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(sys.argv[2])
        sys.exit(0)
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "validity_bench.txt"))
    ap.add_argument("--items", default=",".join(ITEMS))
    a = ap.parse_args()
    lines = ["silhouette of every row, fp32 rows x %d, double sums, %s (tools/validity_bench.py)" % (D, torch.cuda.get_device_name(0))]
    print(lines[0], flush=True)
    for item in a.items.split(","):
        if item not in ITEMS:
            sys.exit("tools/validity_bench.py: unknown item %r" % item)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", item], timeout=280, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        sys.stderr.write(r.stderr[-2000:])
        lines += r.stdout.splitlines()
        if r.returncode != 0:
            sys.exit("tools/validity_bench.py: %s failed (exit status %d); nothing further was started" % (item, r.returncode))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
