"""Membership counts of k-th-neighbour balls at a fixed shape -- Q = 10 000 query rows, N = 50 000 gallery rows with their 5th-neighbour
radii, D = 128, "euclid", rows of tests/_knn_ref.posterior -- two ways:
  fused   Manifold.count with gallery_count: sv_ball_scan; the [Q, N] matrix never exists
  matrix  pairwise_distance (sv_pairdist: the 2 GB matrix), then (d <= r).sum(1) and .sum(0) in torch: two more passes over it
One item per process: the driver starts a fresh child, and in the child both ways run in the same process state, each after its own
warm-up: fused 3 warm-up passes and the median of 7 timings of 5 back-to-back passes, matrix 1 warm-up pass and the median of 3 single
passes.  Every timing ends in a device synchronise.  The child asserts that the two give the same integers.  It also times
LatentIndex.search(k = 1, "euclid") on the same rows in the same process -- the same arithmetic per pair, with a 1-slot list and a merge
where the compare is -- and prints the ratio: information, not a bar.  The bar: the fused scan is not slower than the matrix route
(profiles/quality_bench.txt).  Fails without a GPU.
Usage: python tools/quality_bench.py [--out profiles/quality_bench.txt] | --one count"""
import argparse
import os
import re
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shot_vae_amd as S                                   # noqa: E402
from tests import _knn_ref as R                            # noqa: E402
from tools.knn_bench import timed_ms                       # noqa: E402

Q, N, D, K = 10000, 50000, 128, 5
ITEMS = ("count",)


def one(item):
    assert item == "count", item
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()          # noqa: E731
    g = f32(R.posterior(N, D, 4102)[0])
    q = f32(R.posterior(Q, D, 4100)[0])
    q[:Q // 2] = 0.98 * g[:Q // 2] + 0.02 * q[:Q // 2]       # half of the queries near a gallery row: both outcomes occur
    man = S.Manifold(D, "euclid")
    man.add(g)
    r = man.fit(K)
    P = S.aggregate.partials(-(-Q // 64), N)
    held = torch.zeros(N, dtype=torch.int64, device="cuda")

    def fused():
        return man.count(q, gallery_count=held)

    def matrix():
        m = S.pairwise_distance(q, None, g, None, "euclid") <= r[None, :]
        return m.sum(dim=1), m.sum(dim=0)

    got_q = fused()
    want_q, want_g = matrix()
    assert torch.equal(got_q, want_q) and torch.equal(held, want_g), "fused and matrix counts differ"
    inside = int(got_q.sum())
    del want_q, want_g
    index = man.index
    rows = []
    for name, fn, warm, reps, n in (("fused", fused, 3, 7, 5), ("matrix", matrix, 1, 3, 1),
                                    ("search k=1 euclid", lambda: index.search(q, None, 1), 3, 7, 5)):
        med, lo, hi = timed_ms(fn, warm, reps, n)
        rows.append(med)
        print("%-5s P=%2d  %-17s: %10.3f ms  (min %.3f .. max %.3f; %d x %d passes)" % (item, P, name, med, lo, hi, reps, n), flush=True)
    print("%-5s matrix / fused = %.2f   inside pairs %d of %d, equal integers" % (item, rows[1] / rows[0], inside, Q * N), flush=True)
    print("%-5s fused / search(k = 1, euclid) = %.2f" % (item, rows[0] / rows[2]), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "tools/quality_bench.py measures on an MI355X: no GPU here"
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(sys.argv[2])
        sys.exit(0)
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "quality_bench.txt"))
    a = ap.parse_args()
    lines = ["ball membership counts, Q = %d, N = %d, D = %d, k = %d, euclid, fp32, %s (tools/quality_bench.py)"
             % (Q, N, D, K, torch.cuda.get_device_name(0))]
    print(lines[0], flush=True)
    slower = []
    for item in ITEMS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", item], timeout=600, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        sys.stderr.write(r.stderr[-2000:])
        lines += r.stdout.splitlines()
        if r.returncode != 0:
            sys.exit("tools/quality_bench.py: %s failed (exit status %d); nothing further was started" % (item, r.returncode))
        if float(re.search(r"matrix / fused = ([0-9.]+)", r.stdout).group(1)) < 1.0:
            slower.append(item)
    lines.append("the bar (the fused scan not slower than the matrix route): %s" % ("MISSED" if slower else "met"))
    print(lines[-1])
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
