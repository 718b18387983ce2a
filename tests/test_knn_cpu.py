"""Posterior distances and k-NN search without a GPU: the float64 restatement of tests/_knn_ref.py against the reference's own outputs
(tests/golden/make_dist_goldens.py), its tie / empty-slot / vote rules on hand-made cases, the argument refusals of sv_pairdist,
sv_knn_scan and sv_knn_vote through the library, and the Python layer's errors."""
import os

import numpy as np
import pytest
import torch

import shot_vae_amd as S
from shot_vae_amd import _lib as L
from shot_vae_amd import neighbors as NB
from oracle import smooth_oracle as SO
from tests import _cases as T
from tests import _knn_ref as R
from tests.golden import make_dist_goldens as G

SV_E_ARG, SV_E_SHAPE = -1, -2    # include/shotvae_hip.h
PTR = 4096                       # never dereferenced: a refused call launches nothing
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", G.TAG + ".npz")
# fixture array -> (metric, second operand: the gallery "g" or the queries themselves "q")
PAIRS = {"kl": ("kl", "g"), "klpair": ("kl", "g"), "klvec": ("kl", "q"), "w2": ("w2", "g"), "euclid": ("euclid", "g"),
         "meuclid": ("euclid", "g"), "mcosine": ("cosine", "g")}


def test_fixture_is_small_and_complete():
    g = np.load(FIXTURE)
    assert os.path.getsize(FIXTURE) < 200 * 1024
    assert sorted(g.files) == sorted("%s_%s_%s" % (n, s, d) for n in PAIRS for s in G.SIZES for d in G.DTYPES)
    for size, (n1, n2, _) in G.SIZES.items():
        for dt, np_dt in G.DTYPES.items():
            for name, (_, other) in PAIRS.items():
                a = g["%s_%s_%s" % (name, size, dt)]
                assert a.dtype == np_dt and a.shape == (n1, n2 if other == "g" else n1)


@pytest.mark.parametrize("size", sorted(G.SIZES))
@pytest.mark.parametrize("name", sorted(PAIRS))
def test_restatement_reproduces_the_reference_in_float64(size, name):
    g = np.load(FIXTURE)
    u1, l1, u2, l2 = G.dist_inputs(size, "f64")
    metric, other = PAIRS[name]
    got = R.distances(metric, u1, l1, *((u2, l2) if other == "g" else (u1, l1)))
    e = T.rel_err(got, g["%s_%s_f64" % (name, size)])
    assert e < 1e-12, (name, size, e)
    # the reference's own fp32 run agrees with its float64 run to fp32 accuracy: the fixture's two halves describe one function
    assert T.rel_err(g["%s_%s_f32" % (name, size)], g["%s_%s_f64" % (name, size)]) < 2e-5


def test_restatement_self_distance_is_zero():
    u1, l1, _, _ = G.dist_inputs("l", "f64")
    for metric in ("euclid", "w2"):
        for dt in (np.float32, np.float64):
            assert (np.diag(R.distances(metric, u1, l1, u1, l1, dtype=dt)) == 0).all()
    assert np.abs(np.diag(R.distances("kl", u1, l1, u1, l1))).max() < 1e-12


def test_topk_tie_and_empty_slot_rules():
    d = np.array([[3.0, 1.0, 1.0, np.nan, 0.5, np.inf, 1.0],
                  [np.nan, np.nan, np.inf, np.nan, np.inf, np.inf, np.nan]])
    val, idx = R.topk(d, 5, "euclid", col0=10)
    assert idx[0].tolist() == [14, 11, 12, 16, 10] and val[0].tolist() == [0.5, 1.0, 1.0, 1.0, 3.0]      # ties by the smaller index
    assert idx[1].tolist() == [-1] * 5 and np.isposinf(val[1]).all()                                    # NaN / +inf never enter
    val, idx = R.topk(d, 7, "euclid")                       # k > the valid columns: the tail is empty
    assert idx[0].tolist() == [4, 1, 2, 6, 0, -1, -1] and np.isposinf(val[0, 5:]).all()
    # leave-one-out: global index self0 + i is skipped for row i (here: columns 11 and 12 of the chunk starting at 10)
    val, idx = R.topk(d, 2, "euclid", col0=10, self0=11)
    assert idx[0].tolist() == [14, 12] and idx[1].tolist() == [-1, -1]
    # the cosine is a similarity: largest first, -inf and NaN never enter, empty slots are -inf
    s = np.array([[0.2, 0.9, -np.inf, 0.9, np.nan]])
    val, idx = R.topk(s, 4, "cosine")
    assert idx[0].tolist() == [1, 3, 0, -1] and val[0, :3].tolist() == [0.9, 0.9, 0.2] and np.isneginf(val[0, 3])


def test_vote_and_counter_rules():
    g_label = np.array([0, 2, 2, 7, -1, 1])                 # 7 and -1 are outside [0, 3): no vote
    idx = np.array([[1, 0, 2], [3, 4, -1], [0, 5, 3], [5, 0, 9]])      # 9: outside the gallery
    val = np.array([[0.5, 0.1, 2.0], [0.1, 0.2, np.inf], [1.0, 1.0, 0.0], [0.3, 0.3, 0.1]])
    votes, pred = R.vote(val, idx, g_label, 3)
    assert votes.tolist() == [[1, 0, 2], [0, 0, 0], [1, 1, 0], [1, 1, 0]] and pred.tolist() == [2, -1, 0, 0]      # first maximum; -1
    votes, pred = R.vote(val, idx, g_label, 3, mode=1, tau=0.5)
    assert pred.tolist() == [0, -1, 0, 0]
    assert np.allclose(votes[0], [np.exp(-0.2), 0, np.exp(-1.0) + np.exp(-4.0)], rtol=1e-15)
    assert R.vote(val, idx, g_label, 3, mode=2, tau=1.0)[1].tolist() == [2, -1, 0, 0]
    counts, conf = R.counters(np.array([2, -1, 0, 0]), np.array([2, 1, 5, 1]), 3)
    assert counts.tolist() == [1, 4] and conf.tolist() == [[0, 0, 0], [1, 0, 0], [0, 0, 1]]


@pytest.mark.parametrize("kind,metric", R.EVAL_CASES)
def test_evaluate_knn_inputs_are_decided_in_float64(kind, metric):
    """the inputs of the GPU test's evaluate_knn cases, chosen here: with the CPU oracle's posteriors at most 10 % of the test rows
    have their k-th and (k+1)-th neighbour within 4 tolerances, and the votes cover several classes"""
    g, gl, t, _ = R.eval_images(kind)
    mg, lg = R.eval_oracle_posterior(kind, g)
    mq, lq = R.eval_oracle_posterior(kind, t)
    dec, tol, ref = R.decided_rows(metric, mq, lq, mg, lg, R.EVAL_K)
    pred = R.vote(*R.topk(ref, R.EVAL_K, metric), gl.numpy(), R.EVAL_CLASSES)[1]
    print("FIG %s %s undecided %d tol %.2e distances %.2e .. %.2e" % (kind, metric, int((~dec).sum()), tol, ref.min(), ref.max()))
    assert int((~dec).sum()) <= R.MAX_UNDECIDED
    assert len(set(pred[dec].tolist())) >= 5


# ================================================================================================ argument refusals
def _pairdist(**kw):
    a = dict(metric=L.DIST_KL, q_mu=PTR, q_ls=PTR, Q=3, g_mu=PTR, g_ls=PTR, N=5, D=7, out=PTR, ldo=5)
    a.update(kw)
    return L.lib().sv_pairdist(a["metric"], a["q_mu"], a["q_ls"], a["Q"], a["g_mu"], a["g_ls"], a["N"], a["D"], a["out"], a["ldo"], None)


def _scan(**kw):
    a = dict(metric=L.DIST_KL, q_mu=PTR, q_ls=PTR, Q=3, g_mu=PTR, g_ls=PTR, N=5, D=7, col0=0, self0=-1, k=2, best_val=PTR,
             best_idx=PTR, init=1)
    a.update(kw)
    return L.lib().sv_knn_scan(a["metric"], a["q_mu"], a["q_ls"], a["Q"], a["g_mu"], a["g_ls"], a["N"], a["D"], a["col0"], a["self0"],
                               a["k"], a["best_val"], a["best_idx"], a["init"], None)


def _vote(**kw):
    a = dict(best_val=PTR, best_idx=PTR, Q=3, k=2, g_label=PTR, n_gallery=5, K=10, mode=0, tau=1.0, q_label=PTR, pred=PTR, votes=PTR,
             counts=PTR, confusion=PTR)
    a.update(kw)
    return L.lib().sv_knn_vote(a["best_val"], a["best_idx"], a["Q"], a["k"], a["g_label"], a["n_gallery"], a["K"], a["mode"], a["tau"],
                               a["q_label"], a["pred"], a["votes"], a["counts"], a["confusion"], None)


COMMON = [
    (dict(metric=4), SV_E_ARG, b"metric"), (dict(metric=-1), SV_E_ARG, b"metric"),
    (dict(q_mu=None), SV_E_ARG, b"NULL"), (dict(g_mu=None), SV_E_ARG, b"NULL"),
    (dict(q_ls=None), SV_E_ARG, b"reads ls"), (dict(g_ls=None), SV_E_ARG, b"reads ls"),
    (dict(metric=L.DIST_W2, q_ls=None), SV_E_ARG, b"reads ls"), (dict(metric=L.DIST_W2, g_ls=None), SV_E_ARG, b"reads ls"),
    (dict(Q=0), SV_E_ARG, b"size"), (dict(N=0), SV_E_ARG, b"size"), (dict(D=0), SV_E_ARG, b"size"), (dict(N=-4), SV_E_ARG, b"size")]


@pytest.mark.parametrize("kw,code,word", COMMON + [
    (dict(out=None), SV_E_ARG, b"out is NULL"), (dict(ldo=4), SV_E_SHAPE, b"ldo"), (dict(ldo=0), SV_E_SHAPE, b"ldo")])
def test_pairdist_refuses_bad_arguments_before_any_launch(kw, code, word):
    assert _pairdist(**kw) == code
    assert word in L.lib().sv_last_error() and b"sv_pairdist" in L.lib().sv_last_error()


@pytest.mark.parametrize("kw,code,word", COMMON + [
    (dict(best_val=None), SV_E_ARG, b"list"), (dict(best_idx=None), SV_E_ARG, b"list"),
    (dict(k=0), SV_E_ARG, b"k=0"), (dict(k=257), SV_E_ARG, b"k=257"), (dict(k=-1), SV_E_ARG, b"k=-1"),
    (dict(col0=-1), SV_E_ARG, b"col0"), (dict(self0=-2), SV_E_ARG, b"self0"), (dict(col0=2 ** 63 - 10), SV_E_SHAPE, b"overflows")])
def test_knn_scan_refuses_bad_arguments_before_any_launch(kw, code, word):
    assert _scan(**kw) == code
    assert word in L.lib().sv_last_error() and b"sv_knn_scan" in L.lib().sv_last_error()


@pytest.mark.parametrize("kw,code,word", [
    (dict(best_idx=None), SV_E_ARG, b"NULL"), (dict(g_label=None), SV_E_ARG, b"NULL"),
    (dict(mode=3), SV_E_ARG, b"mode"), (dict(mode=-1), SV_E_ARG, b"mode"),
    (dict(mode=1, best_val=None), SV_E_ARG, b"best_val"), (dict(mode=2, best_val=None), SV_E_ARG, b"best_val"),
    (dict(mode=1, tau=0.0), SV_E_ARG, b"tau"), (dict(mode=1, tau=-1.0), SV_E_ARG, b"tau"), (dict(mode=2, tau=float("inf")), SV_E_ARG, b"tau"),
    (dict(mode=1, tau=float("nan")), SV_E_ARG, b"tau"),
    (dict(pred=None, votes=None, counts=None, confusion=None), SV_E_ARG, b"no output"),
    (dict(q_label=None), SV_E_ARG, b"labels"), (dict(q_label=None, counts=None), SV_E_ARG, b"labels"),
    (dict(Q=0), SV_E_ARG, b"size"), (dict(K=0), SV_E_ARG, b"size"), (dict(n_gallery=0), SV_E_ARG, b"size"),
    (dict(k=0), SV_E_ARG, b"k=0"), (dict(k=257), SV_E_ARG, b"k=257")])
def test_knn_vote_refuses_bad_arguments_before_any_launch(kw, code, word):
    assert _vote(**kw) == code
    assert word in L.lib().sv_last_error() and b"sv_knn_vote" in L.lib().sv_last_error()


def test_refusals_leave_the_valid_forms_alone():
    """what the refusals must NOT catch (checked on the argument list only: a NULL stream and fake pointers cannot be launched here,
    so each of these is probed through a LATER refusal): ls may be NULL for the metrics that ignore it, best_val in mode 0"""
    for m in (L.DIST_EUCLID, L.DIST_COSINE):
        assert _pairdist(metric=m, q_ls=None, g_ls=None, ldo=1) == SV_E_SHAPE and b"ldo" in L.lib().sv_last_error()
        assert _scan(metric=m, q_ls=None, g_ls=None, k=0) == SV_E_ARG and b"k=0" in L.lib().sv_last_error()
    assert _vote(mode=0, best_val=None, tau=0.0, k=0) == SV_E_ARG and b"k=0" in L.lib().sv_last_error()


def test_entry_points_are_bound_and_exported():
    for name in ("sv_pairdist", "sv_knn_scan", "sv_knn_vote"):
        assert name in L.EXPORTS and hasattr(L.lib(), name)
    assert L.lib().sv_version() == L.ABI_VERSION == 8
    for name in ("LatentIndex", "encode_posterior", "pairwise_distance", "KnnEvaluator", "evaluate_knn", "pairwise_norm_kl_dist_gpu",
                 "pairwise_square_euclidean_gpu", "pairwise_norm_wasserstein_dist_gpu", "calculate_mean_dist_pairwise"):
        assert hasattr(S, name)
        assert name in ("KnnEvaluator", "evaluate_knn") or hasattr(NB, name)


# ================================================================================================ the Python layer
def test_python_layer_refuses_cpu_tensors_and_bad_arguments():
    mu, ls = torch.zeros(4, 8), torch.zeros(4, 8)
    lab = torch.zeros(4, dtype=torch.int64)
    calls = [lambda: NB.pairwise_distance(mu, ls, mu, ls), lambda: NB.pairwise_norm_kl_dist_gpu(mu, ls, mu, ls),
             lambda: NB.pairwise_square_euclidean_gpu(mu, mu), lambda: NB.pairwise_norm_wasserstein_dist_gpu(mu, ls, mu, ls),
             lambda: NB.calculate_mean_dist_pairwise(mu, mu, GPU_flag=False), lambda: NB.LatentIndex(8).add(mu, ls, lab),
             lambda: NB.LatentIndex(8).search(mu, ls, 3), lambda: NB.LatentIndex(8, num_classes=3).classify(mu, ls, 3)]
    for fn in calls:
        with pytest.raises(L.ShotVaeHipError, match="MI355X|no CPU fallback"):
            fn()
    with pytest.raises(NotImplementedError, match="distance manhattan not implemented"):
        NB.calculate_mean_dist_pairwise(mu, mu, distance="manhattan")
    with pytest.raises(NotImplementedError, match="distance manhattan not implemented"):
        NB.calculate_mean_dist_pairwise(mu, mu, GPU_flag=False, distance="manhattan")
    for fn in (lambda: NB.pairwise_distance(mu, ls, mu, ls, metric="manhattan"), lambda: NB.LatentIndex(8, metric="manhattan"),
               lambda: S.evaluate_knn(None, [], [], metric="manhattan", num_classes=3)):
        with pytest.raises(ValueError, match="unknown metric"):
            fn()
    for k in (0, 257, -3):
        with pytest.raises(ValueError, match=r"k must be in \[1, 256\]"):
            NB.LatentIndex(8).search(mu, ls, k)
        with pytest.raises(ValueError, match=r"k must be in \[1, 256\]"):
            NB.LatentIndex(8, num_classes=3).classify(mu, ls, k)
    with pytest.raises(ValueError, match="num_classes"):
        NB.LatentIndex(8).classify(mu, ls, 3)
    with pytest.raises(ValueError, match="weights"):
        NB.LatentIndex(8, num_classes=3).classify(mu, ls, 3, weights="rank")
    assert len(NB.LatentIndex(8)) == 0


def test_encode_posterior_is_eval_mode_only_and_refuses_cpu_tensors():
    x = torch.zeros(2, 3, 32, 32)
    vae = S.VariationalAutoEncoder("wideresnet-10-1", num_input_channels=3, img_size=(32, 32), data_parallel=False,
                                   continuous_latent_dim=128, disc_latent_dim=10, small_input=True, compute_dtype="fp32")
    smooth = S.SmoothVAE((SO.KINDS["svhn"]["in_ch"], 32, 32), {"cont": 32, "disc": [10]}, compute_dtype="fp32")
    for m in (vae, smooth):
        m.train()
        with pytest.raises(NotImplementedError, match="eval mode only"):
            S.encode_posterior(m, x)
        with pytest.raises(NotImplementedError, match="eval mode only"):
            S.evaluate_knn(m, [(x, torch.zeros(2, dtype=torch.int64))], [], num_classes=10)
        m.eval()
        with pytest.raises(L.ShotVaeHipError, match="MI355X"):
            S.encode_posterior(m, x)
        assert not m.training
    with pytest.raises(TypeError, match="VariationalAutoEncoder or a SmoothVAE"):
        S.encode_posterior(torch.nn.Linear(2, 2), x)
