"""The calibration module at the sizes of a test set -- SVHN's 26 032 x 10 classes, CIFAR-100's 10 000 x 100 -- against the usual torch
formulations, each in the same process state:
  rel     Reliability: sv_calib_rows + sv_calib_accum + sv_calib_finish (update + reduce, no host read) against log_softmax / max /
          bucketize / bincount / index_add_ (torch.bincount reads the host: that way cannot be captured), eager and replayed from a graph
  fit     TemperatureScaler.fit(iters=12) -- 24 launches and one host read -- against torch.optim.LBFGS on the same NLL (lr 0.01, 50
          iterations: the recipe of Guo et al.'s reference code); both end with the temperature on the host
  detect  detection_metrics (AUROC, AUPR both ways, FPR at 95 % TPR; two sv_rank_scan passes, O(n^2) comparisons) at 26 032 + 26 032
          scores against an AUROC from one torch.sort (O(n log n); a tie is ranked one way or the other), and sv_rank_scan on its own
One item per process: the driver starts a fresh child for each, one after the other, and stops at the first that fails.  In a child every
way runs after its own warm-up (3 passes): the median of 7 timings of 20 back-to-back passes, each timing ending in a device synchronise.
The child asserts that the two ways agree.  No ratio is required: the file records what was measured (profiles/calibration_bench.txt).
Fails without a GPU.
Usage: python tools/calibration_bench.py [--out profiles/calibration_bench.txt] [--items rel:26032x10,...] | --one ITEM"""
import argparse
import os
import subprocess
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shot_vae_amd as S                                   # noqa: E402
from tools.cluster_bench import graphed                    # noqa: E402
from tools.knn_bench import timed_ms                       # noqa: E402

ITEMS = ("rel:26032x10", "rel:10000x100", "fit:26032x10", "fit:10000x100", "detect:26032+26032")
WARM, REPS, PASSES = 3, 7, 20
BINS = 15


def logits(n, k, seed=0):
    """normal logits of scale 3, 70 % of the labels at the argmax: an over-confident classifier"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = 3.0 * torch.randn(n, k, device="cuda", generator=g)
    at = torch.rand(n, device="cuda", generator=g) < 0.7
    return x, torch.where(at, x.argmax(1), torch.randint(0, k, (n,), device="cuda", generator=g))


def torch_reliability(x, label, inner):
    lp = torch.log_softmax(x, dim=1)
    lconf, pred = lp.max(dim=1)
    conf, p = lconf.exp(), lp.exp()
    nll = -lp.gather(1, label[:, None]).squeeze(1)
    brier = ((p - F.one_hot(label, x.shape[1])) ** 2).sum(dim=1)
    entropy = -(p * lp).sum(dim=1)
    b = torch.bucketize(conf, inner)                       # the number of inner edges below conf: (lo, hi] bins
    hit = (pred == label).double()
    count = torch.bincount(b, minlength=BINS).double()
    acc = torch.bincount(b, weights=hit, minlength=BINS) / count
    mean = torch.zeros(BINS, dtype=torch.float64, device=x.device).index_add_(0, b, conf.double()) / count
    gap = torch.nan_to_num((acc - mean).abs())
    n = float(x.shape[0])
    return torch.stack([hit.sum() / n, conf.double().sum() / n, (count / n * gap).sum(), gap.max(), nll.double().sum() / n,
                        brier.double().sum() / n, entropy.double().sum() / n])


def report(tag, runs):
    got = {}
    for name, fn in runs:
        if fn is None:
            continue
        med, lo, hi = timed_ms(fn, WARM, REPS, PASSES)
        got[name] = med
        print("%-18s %-18s: %9.4f ms  (min %.4f .. max %.4f; %d x %d passes)" % (tag, name, med, lo, hi, REPS, PASSES), flush=True)
    return got


def ratio(tag, got, ours, theirs):
    if ours in got and theirs in got:
        print("%-18s %s / %s = %.2f" % (tag, theirs, ours, got[theirs] / got[ours]), flush=True)


def one_rel(tag, n, k):
    x, label = logits(n, k)
    rel = S.Reliability(k, bins=BINS).reserve(n, x.device)
    inner = rel.edges[1:-1].to(x.device)

    def ours():
        rel.n = 0
        rel.update(x, label)
        return rel.reduce()[0]

    def theirs():
        return torch_reliability(x, label, inner)

    a, b = ours()[:7].double(), theirs()
    err = float((a - b).abs().max())
    assert err <= 1e-5, "Reliability and the torch formulation disagree by %g: %s against %s" % (err, a.tolist(), b.tolist())
    got = report(tag, [("ours eager", ours), ("ours graph", graphed(ours)), ("torch eager", theirs), ("torch graph", graphed(theirs))])
    ratio(tag, got, "ours eager", "torch eager")
    ratio(tag, got, "ours graph", "torch eager")
    print("%-18s max |difference| of the seven scalars = %.1e   ece = %.6f" % (tag, err, float(a[2])), flush=True)


def one_fit(tag, n, k):
    x, label = logits(n, k)

    def ours():
        return float(S.TemperatureScaler().fit(x, label, iters=12).temperature.cpu()[0])

    def theirs():
        t = torch.nn.Parameter(torch.ones(1, device=x.device))
        opt = torch.optim.LBFGS([t], lr=0.01, max_iter=50)

        def closure():
            opt.zero_grad()
            loss = F.cross_entropy(x / t, label)
            loss.backward()
            return loss

        opt.step(closure)
        return float(t.detach().cpu()[0])

    nll = lambda t: float(F.cross_entropy(x.double() / t, label))          # noqa: E731
    ta, tb = ours(), theirs()
    assert nll(ta) <= nll(tb) + 1e-9, "the Newton fit ends above LBFGS: T = %g (NLL %g) against %g (%g)" % (ta, nll(ta), tb, nll(tb))
    got = report(tag, [("ours fit(12)", ours), ("torch LBFGS(50)", theirs)])
    ratio(tag, got, "ours fit(12)", "torch LBFGS(50)")
    print("%-18s T = %.6f (NLL %.7f) against LBFGS T = %.6f (NLL %.7f); NLL at T = 1: %.7f" % (tag, ta, nll(ta), tb, nll(tb), nll(1.0)),
          flush=True)


def one_detect(tag, n_pos, n_neg):
    g = torch.Generator(device="cuda").manual_seed(0)
    score = torch.cat([0.5 + torch.randn(n_pos, device="cuda", generator=g), -0.5 + torch.randn(n_neg, device="cuda", generator=g)])
    positive = torch.cat([torch.ones(n_pos, dtype=torch.int64), torch.zeros(n_neg, dtype=torch.int64)]).cuda()
    perm = torch.randperm(n_pos + n_neg, device="cuda", generator=g)
    score, positive = score[perm].contiguous(), positive[perm].contiguous()

    def ours():
        return S.detection_metrics(score, positive)

    def theirs():                                          # the rank-sum AUROC: exact only without ties
        rank = torch.empty_like(perm)
        rank[torch.sort(score).indices] = torch.arange(1, score.numel() + 1, device=score.device)
        return (rank[positive == 1].double().sum() - n_pos * (n_pos + 1) / 2.0) / (float(n_pos) * n_neg)

    def scan():
        return S.rank_counts(score, score, positive)

    # (52 064 fp32 normals hold a few dozen tied pairs; the sort ranks a tie one way or the other, 0.5 / (n_pos n_neg) = 7e-10 each)
    a, b = float(ours().auroc), float(theirs())
    assert abs(a - b) <= 1e-6, "AUROC %.12f against the sort's %.12f" % (a, b)
    got = report(tag, [("ours eager", ours), ("ours graph", graphed(ours)), ("torch sort AUROC", theirs), ("one sv_rank_scan", scan)])
    ratio(tag, got, "ours eager", "torch sort AUROC")
    print("%-18s AUROC = %.9f (both ways agree to %.1e)" % (tag, a, abs(a - b)), flush=True)


def one(item):
    what, size = item.split(":")
    if what == "detect":
        one_detect(item, *[int(v) for v in size.split("+")])
    else:
        n, k = (int(v) for v in size.split("x"))
        (one_rel if what == "rel" else one_fit)(item, n, k)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "tools/calibration_bench.py measures on an MI355X: no GPU here"
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(sys.argv[2])
        sys.exit(0)
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "calibration_bench.txt"))
    ap.add_argument("--items", default=",".join(ITEMS))
    a = ap.parse_args()
    lines = ["calibration, temperature scaling and detection metrics, fp32, %s (tools/calibration_bench.py)" % torch.cuda.get_device_name(0)]
    print(lines[0], flush=True)
    for item in a.items.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", item], timeout=300, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        sys.stderr.write(r.stderr[-2000:])
        lines += r.stdout.splitlines()
        if r.returncode != 0:
            sys.exit("tools/calibration_bench.py: %s failed (exit status %d); nothing further was started" % (item, r.returncode))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
