"""Generate the posterior-distance fixture by running the REFERENCE's lib/utils/calculate_dist.py on CPU (sibling of the other
make_*_goldens.py scripts: the reference is imported from its checkout at generation time, the inputs are closed forms of
oracle/closed_form.py, the fixture holds the reference's OUTPUTS only).

For (n1, n2, d) = (7, 5, 6) ["s"] and (33, 65, 128) ["l"], in fp32 ["f32"] and float64 ["f64"], on the inputs of dist_inputs():
  kl_*         pairwise_norm_kl_dist_gpu(u1, ls1, u2, ls2)                       [n1, n2]   (torch, on CPU tensors)
  euclid_*     pairwise_square_euclidean_gpu(u1, u2)                             [n1, n2]
  w2_*         pairwise_norm_wasserstein_dist_gpu(u1, ls1, u2, ls2)              [n1, n2]
  klvec_*      gaussian_kl_calculation_vec(u1, ls1, GPU_flag=False)              [n1, n1]   (numpy)
  klpair_*     gaussian_kl_calculation_vec_pairwise(u1, ls1, u2, ls2, False)     [n1, n2]   (numpy)
  meuclid_*    calculate_mean_dist_pairwise(u1, u2, GPU_flag=False, "euclidean") [n1, n2]   (numpy)
  mcosine_*    calculate_mean_dist_pairwise(u1, u2, GPU_flag=False, "cosine")    [n1, n2]   (numpy)
keys are "<name>_<size>_<dtype>".

    python tests/golden/make_dist_goldens.py

Writes tests/golden/ref_calculate_dist.npz.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import numpy as np                            # noqa: E402
from oracle import closed_form as C           # noqa: E402

TAG = "ref_calculate_dist"
SIZES = {"s": (7, 5, 6), "l": (33, 65, 128)}
DTYPES = {"f32": np.float32, "f64": np.float64}
STREAM = 9900


def posterior(n, d, stream):
    """closed-form rows: mu ~ N(0, 1), log sigma ~ U(-1, 0.5), fp32 values (as float64 arrays)"""
    mu = C.normal((n, d), stream).numpy().astype(np.float64)
    ls = C.uniform((n, d), stream + 1, -1.0, 0.5).numpy().astype(np.float64)
    return mu, ls


def dist_inputs(size, dtype="f64"):
    """(u1, ls1, u2, ls2) of the fixture's case `size`: fp32-representable values in the requested dtype"""
    n1, n2, d = SIZES[size]
    base = STREAM + 10 * sorted(SIZES).index(size)
    u1, l1 = posterior(n1, d, base)
    u2, l2 = posterior(n2, d, base + 2)
    return tuple(a.astype(DTYPES[dtype]) for a in (u1, l1, u2, l2))


def run():
    import torch
    sys.path.insert(0, HERE)
    import make_goldens as MG
    assert os.path.isdir(MG.REF), "reference not mounted; goldens are generated in the build container"
    sys.path.insert(0, MG.REF)
    from lib.utils import calculate_dist as R
    out = {}
    for size in SIZES:
        for dt in DTYPES:
            u1, l1, u2, l2 = dist_inputs(size, dt)
            t = [torch.from_numpy(a) for a in (u1, l1, u2, l2)]
            key = "_%s_%s" % (size, dt)
            out["kl" + key] = R.pairwise_norm_kl_dist_gpu(*t).numpy()
            out["euclid" + key] = R.pairwise_square_euclidean_gpu(t[0], t[2]).numpy()
            out["w2" + key] = R.pairwise_norm_wasserstein_dist_gpu(*t).numpy()
            out["klvec" + key] = R.gaussian_kl_calculation_vec(u1, l1, GPU_flag=False)
            out["klpair" + key] = R.gaussian_kl_calculation_vec_pairwise(u1, l1, u2, l2, GPU_flag=False)
            out["meuclid" + key] = R.calculate_mean_dist_pairwise(u1, u2, GPU_flag=False, distance="euclidean")
            out["mcosine" + key] = R.calculate_mean_dist_pairwise(u1, u2, GPU_flag=False, distance="cosine")
            for k in list(out):
                if k.endswith(key):
                    assert out[k].dtype == DTYPES[dt], (k, out[k].dtype)
    path = os.path.join(HERE, TAG + ".npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    run()
