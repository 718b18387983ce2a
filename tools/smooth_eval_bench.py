"""Test accuracy of a smooth-ELBO model (svhn_VAE, bf16) over 26 032 synthetic images -- the size of the SVHN test split -- in batches
of 1 024 (25 full batches and one of 432), two ways:
  parent           what Trainer.eval (main_smooth_ELBO_svhn.py:217-226) does with the library as it was: eval-mode model(x) (encoder,
                   sampler, decoder, Tanh), torch argmax of alpha, and one host read per batch (.cpu().numpy()) to count the hits
  evaluate_smooth  shot_vae_amd.evaluate_smooth: encoder + sv_smooth_classify, the counters on the device, one host read at the end
Both count the same hits (asserted).  The method of tools/infer_bench.py: one item per process -- the driver starts a fresh child for
each, one after the other, and stops at the first that fails; in a child 5 warm-up passes, then the median of 7 timings of n
back-to-back passes (n: at least 20, and enough for a quarter of a second per timing), min .. max beside it.  The driver prints the
ratio parent / evaluate_smooth.  There is no target: the figures are a record (profiles/smooth_eval_bench.txt).  Fails without a GPU.
Usage: python tools/smooth_eval_bench.py [--one ITEM]"""
import os
import re
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shot_vae_amd as S                                   # noqa: E402
from tools.infer_bench import timed_ms                      # noqa: E402

ITEMS = ("parent", "evaluate_smooth")
IMAGES, B = 26032, 1024


def one(item):
    torch.manual_seed(0)
    m = S.SmoothVAE((3, 32, 32), {"cont": 32, "disc": [10]}, compute_dtype="bf16").cuda()
    with torch.no_grad():
        m.fc_alphas[0].weight.mul_(400.0)                  # spread the predictions over the classes (the default head is near uniform)
    x = torch.rand(IMAGES, 3, 32, 32, device="cuda") * 2.0 - 1.0
    label = torch.randint(0, 10, (IMAGES,), device="cuda")
    batches = [(x[i:i + B], label[i:i + B]) for i in range(0, IMAGES, B)]
    if item == "parent":
        m.eval()

        def call():
            count = 0
            with torch.no_grad():
                for image, y in batches:
                    dist = m(image)[1]
                    pre = torch.max(dist["disc"][0], 1)[1].cpu().numpy()
                    count += np.sum(pre == y.cpu().numpy())
            return int(count)
    else:
        call = lambda: S.evaluate_smooth(m, batches)["correct"]
    med, lo, hi, n = timed_ms(call)
    hits = call()
    m.eval()
    with torch.no_grad():
        want = sum(int((m(image)[1]["disc"][0].argmax(1) == y).sum()) for image, y in batches)
    assert hits == want, (item, hits, want)
    print("svhn_VAE bf16, %d images at B = %d, %-15s: %8.3f ms per pass  (min %.3f .. max %.3f; 7 x %3d passes)  %9.0f images/s  hits %d"
          % (IMAGES, B, item, med, lo, hi, n, IMAGES / med * 1e3, hits), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "tools/smooth_eval_bench.py measures on an MI355X: no GPU here"
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(sys.argv[2])
        sys.exit(0)
    ms = {}
    for item in ITEMS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", item], timeout=300, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            sys.exit("tools/smooth_eval_bench.py: %s failed (exit status %d); nothing further was started" % (item, r.returncode))
        ms[item] = float(re.search(r":\s+([0-9.]+) ms per pass", r.stdout).group(1))
    print("parent / evaluate_smooth = %.2f" % (ms["parent"] / ms["evaluate_smooth"]))
