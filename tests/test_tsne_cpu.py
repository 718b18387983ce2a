"""t-SNE without a GPU: the float64 restatement of tests/_tsne_ref.py against scikit-learn's private kernels (the bisection, the KL and
its gradient) and against finite differences of its own KL; symmetrize and pca_project (plain torch) on CPU tensors against the dense
forms; the argument refusals of the four entry points of csrc/tsne.hip through the library (refused before any HIP call, so they need no
device); the Python layer's errors (shot_vae_amd.embed)."""
import numpy as np
import pytest
import torch

import shot_vae_amd as S
from shot_vae_amd import _lib as L
from shot_vae_amd import embed as E
from oracle import smooth_oracle as SO
from tests import _tsne_ref as R

SV_E_ARG, SV_E_SHAPE = -1, -2    # include/shotvae_hip.h
PTR = 4096                       # never dereferenced: a refused call launches nothing


def lists(n, k, seed, scale=1.0, dim=6):
    """the k-lists of n random points (float64 squared Euclid distances x scale, as fp32 values)"""
    x = np.random.default_rng(seed).normal(size=(n, dim))
    d, idx = R.knn_lists(x, k)
    return (d * scale).astype(np.float32).astype(np.float64), idx


# ================================================================================================ against scikit-learn
SEARCH_CASES = [(130, 20, 5.0, 1.0, 11), (257, 90, 30.0, 1.0, 12), (65, 5, 2.0, 1.0, 13), (300, 256, 80.0, 1.0, 14),
                (130, 20, 5.0, 1e-6, 11), (130, 20, 5.0, 1e6, 11), (130, 20, 5.0, 1.0, 11)]


@pytest.mark.parametrize("n,k,perplexity,scale,seed", SEARCH_CASES)
def test_conditional_affinities_match_scikit_learn(n, k, perplexity, scale, seed):
    U = pytest.importorskip("sklearn.manifold._utils")
    if not hasattr(U, "_binary_search_perplexity"):
        pytest.skip("sklearn.manifold._utils._binary_search_perplexity is gone")
    d, idx = lists(n, k, seed, scale)
    want = np.asarray(U._binary_search_perplexity(d.astype(np.float32), perplexity, 0), dtype=np.float64)
    p, beta, steps = R.conditional(d, idx, perplexity)
    err = float(np.abs(p - want).max())
    print("FIG search %s err %.3e steps <= %d" % ((n, k, perplexity, scale), err, int(steps.max())))
    assert err <= 1e-5
    assert steps.max() < 100, "a row met the cap"
    assert np.allclose(p.sum(axis=1), 1.0, atol=1e-12)
    for i in range(0, n, 17):                          # the returned beta is the beta of p, and meets the tolerance
        assert np.array_equal(R.softmax_row(d[i], np.ones(k, bool), beta[i]), p[i])
        assert abs(R.entropy(p[i]) - np.log(perplexity)) <= 1e-5 + 1e-12


@pytest.mark.parametrize("n,d,seed", [(40, 2, 21), (33, 3, 22)])
def test_gradient_and_kl_match_scikit_learn(n, d, seed):
    T = pytest.importorskip("sklearn.manifold._t_sne")
    squareform = pytest.importorskip("scipy.spatial.distance").squareform
    if not hasattr(T, "_kl_divergence"):
        pytest.skip("sklearn.manifold._t_sne._kl_divergence is gone")
    dist, idx = lists(n, 12, seed)
    P = R.joint_dense(R.conditional(dist, idx, 4.0)[0], idx)
    y = np.random.default_rng(seed + 1).normal(size=(n, d))
    want_kl, want_g = T._kl_divergence(y.ravel(), squareform(P, checks=False), 1.0, n, d)
    g, kl, _ = R.gradient(P, y)
    print("FIG sklearn kl %.3e grad %.3e" % (abs(kl - want_kl), float(np.abs(g.ravel() - want_g).max())))
    assert abs(kl - want_kl) <= 1e-12
    assert float(np.abs(g.ravel() - want_g).max()) <= 1e-12


# ================================================================================================ always
@pytest.mark.parametrize("n,d,e", [(30, 2, 1.0), (25, 3, 1.0)])
def test_gradient_is_the_derivative_of_the_kl(n, d, e):
    dist, idx = lists(n, 10, 31)
    P = R.joint_dense(R.conditional(dist, idx, 3.0)[0], idx)
    y = np.random.default_rng(32).normal(size=(n, d))
    g = R.gradient(P, y, e)[0]
    h = 1e-5
    for i, c in ((0, 0), (7, d - 1), (n - 1, 1)):
        hi, lo = y.copy(), y.copy()
        hi[i, c] += h
        lo[i, c] -= h
        fd = (R.kl(P, hi) - R.kl(P, lo)) / (2 * h)
        assert abs(fd - g[i, c]) <= 1e-8 + 1e-6 * abs(g[i, c]), (i, c, fd, g[i, c])
    assert np.abs(g.sum(axis=0)).max() <= 1e-14 * np.abs(g).sum()
    # the exaggeration scales the attraction alone
    A = R.attraction(P, y)[0]
    assert np.allclose(R.gradient(P, y, 12.0)[0] - g, 4.0 * 11.0 * A, rtol=1e-12, atol=1e-15)


def test_joint_is_symmetric_and_sums_to_one():
    dist, idx = lists(50, 9, 41)
    idx = idx.copy()
    idx[3, 4:] = -1                                    # a short list
    p = R.conditional(dist, idx, 3.0)[0]
    assert (p[3, 4:] == 0).all() and abs(p[3].sum() - 1) < 1e-12
    P = R.joint_dense(p, idx)
    assert np.array_equal(P, P.T) and abs(P.sum() - 1.0) < 1e-12 and (np.diag(P) == 0).all()


def test_restatement_search_rules():
    d = np.array([1.0, 1.0, 1.0, 1.0, 1.0])
    p, beta, steps = R.search_row(d, np.ones(5, bool), 2.0, max_steps=100)           # all equal: H = log 5 whatever beta
    assert steps == 100 and np.array_equal(p, np.full(5, 0.2)) and beta == 2.0 ** 99
    p, beta, steps = R.search_row(d, np.array([False, True, False, False, False]), 2.0)
    assert p.tolist() == [0, 1, 0, 0, 0] and beta == 1.0 and steps == 100
    p, _, steps = R.search_row(d, np.zeros(5, bool), 2.0)
    assert p.sum() == 0 and steps == 100
    d = np.array([0.5, np.inf, 0.7, np.nan, 1.5, 2.0])
    ok = R.valid_slots(d[None], np.array([[1, 2, 3, 4, -1, 6]]))[0]
    assert ok.tolist() == [True, False, True, False, False, True]
    p, beta, steps = R.search_row(d, ok, 2.0)
    assert steps < 100 and (p[~ok] == 0).all() and abs(R.entropy(p) - np.log(2.0)) <= 1e-5


def test_update_rule():
    y, vel, gain = np.zeros(5), np.array([1.0, -1.0, 0.0, 1.0, 1.0]), np.array([1.0, 1.0, 1.0, 0.012, 0.0125])
    g = np.array([-2.0, -2.0, 3.0, 1.0, 1.0])
    y1, v1, k1 = R.update(y, vel, gain, g, 0.5, 10.0)
    assert np.allclose(k1, [1.2, 0.8, 0.8, 0.01, 0.01]) and k1[3] == 0.01           # inc, dec, vel g == 0 decays, the floor
    assert np.allclose(v1, 0.5 * vel - 10.0 * k1 * g) and np.array_equal(y1, v1)


# ================================================================================================ symmetrize, pca_project
def test_symmetrize_matches_the_dense_form():
    # row 0 <-> 1 mutual; 2 -> 0 one way; row 3 is a hub (every row lists it); -1 slots and a zero
    idx = torch.tensor([[1, 3, -1], [0, 3, -1], [0, 3, 4], [-1, -1, -1], [3, 2, -1], [3, -1, -1]])
    p = torch.tensor([[.7, .3, .9], [.6, .4, 0], [.5, .25, .25], [.1, .2, .3], [1.0, 0.0, 0], [1.0, 0, 0]], dtype=torch.float32)
    rowptr, col, val = S.symmetrize(p, idx)
    n = 6
    dense = np.zeros((n, n))
    for i in range(n):
        lo, hi = int(rowptr[i]), int(rowptr[i + 1])
        assert col[lo:hi].tolist() == sorted(set(col[lo:hi].tolist())), "columns ascending and distinct"
        dense[i, col[lo:hi].numpy()] = val[lo:hi].double().numpy()
    pv = np.where(idx.numpy() >= 0, p.double().numpy(), 0.0)
    want = R.joint_dense(pv, idx.numpy())
    assert rowptr[0] == 0 and int(rowptr[-1]) == col.numel() == val.numel() == int((want > 0).sum())
    assert np.abs(dense - want).max() <= 2.0 ** -24 * want.max() and np.array_equal(dense, dense.T)
    assert int(rowptr[4] - rowptr[3]) == 5, "the hub has every other row"
    assert rowptr.dtype == col.dtype == torch.int64 and val.dtype == torch.float32
    # no edge at all
    rowptr, col, val = S.symmetrize(torch.zeros(3, 2), torch.full((3, 2), -1, dtype=torch.int64))
    assert rowptr.tolist() == [0, 0, 0, 0] and col.numel() == 0 and val.numel() == 0
    # a real k-list: sums to 1
    dist, ix = lists(70, 8, 51)
    pc = R.conditional(dist, ix, 3.0)[0]
    rowptr, col, val = S.symmetrize(torch.from_numpy(pc).float(), torch.from_numpy(ix))
    assert abs(float(val.double().sum()) - 1.0) < 1e-6
    with pytest.raises(ValueError):
        S.symmetrize(torch.zeros(3, 2), torch.zeros(3, 3, dtype=torch.int64))


@pytest.mark.parametrize("n,D,d", [(50, 7, 2), (40, 5, 3)])
def test_pca_project_matches_numpy(n, D, d):
    x = np.random.default_rng(61).normal(size=(n, D)) * np.arange(1, D + 1)
    xc = x - x.mean(axis=0)
    w, v = np.linalg.eigh(xc.T @ xc / (n - 1))
    v = v[:, ::-1][:, :d]
    for c in range(d):
        if v[np.argmax(np.abs(v[:, c])), c] < 0:
            v[:, c] = -v[:, c]
    want = xc @ v
    want = want / np.std(want[:, 0]) * 1e-4
    got = S.pca_project(torch.from_numpy(x).float(), d)
    assert got.dtype == torch.float64 and tuple(got.shape) == (n, d)
    assert np.abs(got.numpy() - want).max() <= 1e-6 * 1e-4 * 10          # (x enters as fp32)
    got64 = S.pca_project(torch.from_numpy(x), d).numpy()
    assert np.abs(got64 - want).max() <= 1e-12 and abs(np.std(got64[:, 0]) - 1e-4) < 1e-15
    with pytest.raises(ValueError):
        S.pca_project(torch.zeros(4, 3), 4)


# ================================================================================================ argument refusals
def _affinity(**kw):
    a = dict(dist=PTR, idx=PTR, N=5, k=20, perplexity=5.0, tol=1e-5, max_steps=100, p=PTR, beta=PTR, steps=PTR)
    a.update(kw)
    return L.lib().sv_tsne_affinity(a["dist"], a["idx"], a["N"], a["k"], a["perplexity"], a["tol"], a["max_steps"], a["p"], a["beta"],
                                    a["steps"], None)


def _attract(**kw):
    a = dict(y=PTR, N=5, d=2, rowptr=PTR, col=PTR, val=PTR, attr=PTR, rowkl=PTR)
    a.update(kw)
    return L.lib().sv_tsne_attract(a["y"], a["N"], a["d"], a["rowptr"], a["col"], a["val"], a["attr"], a["rowkl"], None)


def _repulse(**kw):
    a = dict(y=PTR, N=5, d=2, P=2, rep=PTR, z=PTR)
    a.update(kw)
    return L.lib().sv_tsne_repulse(a["y"], a["N"], a["d"], a["P"], a["rep"], a["z"], None)


def _update(**kw):
    a = dict(y=PTR, vel=PTR, gain=PTR, attr=PTR, rowkl=PTR, rep=PTR, z=PTR, P=2, N=5, d=2, hyper=PTR, scratch=PTR, stats=PTR)
    a.update(kw)
    return L.lib().sv_tsne_update(a["y"], a["vel"], a["gain"], a["attr"], a["rowkl"], a["rep"], a["z"], a["P"], a["N"], a["d"], a["hyper"],
                                  a["scratch"], a["stats"], None)


DIMS = [(dict(d=1), SV_E_SHAPE, b"d=1"), (dict(d=4), SV_E_SHAPE, b"d=4")]
SIZES = [(dict(N=0), SV_E_ARG, b"size"), (dict(N=-3), SV_E_ARG, b"size")]
STATES = [(dict(P=0), SV_E_ARG, b"P=0"), (dict(P=65), SV_E_ARG, b"P=65")]


@pytest.mark.parametrize("fn,name,cases", [
    (_affinity, b"sv_tsne_affinity",
     [(dict([(k, None)]), SV_E_ARG, b"NULL") for k in ("dist", "idx", "p", "beta", "steps")] + SIZES
     + [(dict(k=0), SV_E_ARG, b"k=0"), (dict(k=257, perplexity=30.0), SV_E_ARG, b"k=257"), (dict(perplexity=1.0), SV_E_ARG, b"perplexity"),
        (dict(perplexity=0.5), SV_E_ARG, b"perplexity"), (dict(perplexity=20.0), SV_E_ARG, b"perplexity"),
        (dict(perplexity=21.0), SV_E_ARG, b"perplexity"), (dict(perplexity=float("nan")), SV_E_ARG, b"perplexity"),
        (dict(k=1, perplexity=1.5), SV_E_ARG, b"perplexity"), (dict(tol=-1.0), SV_E_ARG, b"tol"), (dict(max_steps=0), SV_E_ARG, b"max_steps")]),
    (_attract, b"sv_tsne_attract",
     [(dict([(k, None)]), SV_E_ARG, b"NULL") for k in ("y", "rowptr", "attr", "rowkl")] + SIZES + DIMS),
    (_repulse, b"sv_tsne_repulse",
     [(dict([(k, None)]), SV_E_ARG, b"NULL") for k in ("y", "rep", "z")] + SIZES + DIMS + STATES),
    (_update, b"sv_tsne_update",
     [(dict([(k, None)]), SV_E_ARG, b"NULL") for k in ("y", "vel", "gain", "attr", "rowkl", "rep", "z", "hyper", "scratch", "stats")]
     + SIZES + DIMS + STATES),
])
def test_entry_points_refuse_bad_arguments_before_any_launch(fn, name, cases):
    for kw, code, word in cases:
        assert fn(**kw) == code, (name, kw)
        err = L.lib().sv_last_error()
        assert word in err and name in err, (kw, err)


def test_entry_points_are_bound_and_exported():
    for name in ("sv_tsne_affinity", "sv_tsne_attract", "sv_tsne_repulse", "sv_tsne_update"):
        assert name in L.EXPORTS and hasattr(L.lib(), name)
    assert L.lib().sv_version() == L.ABI_VERSION == 8
    for name in ("TSNE", "conditional_affinities", "symmetrize", "pca_project", "evaluate_embedding"):
        assert getattr(S, name) is getattr(E, name)
    assert E.repulse_partials(50000) == 6 and E.repulse_partials(64) == 1 and E.repulse_partials(1000) == 16
    assert E.update_scratch(1) == 3 and E.update_scratch(257) == 6


# ================================================================================================ the Python layer
def test_python_layer_errors():
    mu = torch.zeros(200, 8)
    with pytest.raises(ValueError, match="cosine"):
        S.TSNE(metric="cosine")
    with pytest.raises(ValueError, match="below k"):
        S.TSNE(perplexity=30.0, k=30)
    with pytest.raises(ValueError, match="below k"):
        S.TSNE(perplexity=30.0).fit(torch.zeros(20, 8))            # the default k is N - 1 = 19
    with pytest.raises(ValueError, match="n_components"):
        S.TSNE(n_components=4)
    with pytest.raises(ValueError, match="init"):
        S.TSNE(init="spectral")
    with pytest.raises(ValueError, match=r"k must be"):
        S.TSNE(k=257)
    with pytest.raises(L.ShotVaeHipError, match="MI355X"):
        S.TSNE().fit(mu)
    with pytest.raises(L.ShotVaeHipError, match="MI355X"):
        S.TSNE(init=torch.zeros(200, 2))
    with pytest.raises(L.ShotVaeHipError, match="MI355X"):
        S.conditional_affinities(torch.zeros(5, 20), torch.zeros(5, 20, dtype=torch.int64), 5.0)
    for perplexity in (1.0, 20.0):
        with pytest.raises(ValueError, match="perplexity"):
            S.conditional_affinities(torch.zeros(5, 20), torch.zeros(5, 20, dtype=torch.int64), perplexity)
    with pytest.raises(ValueError, match="k must be"):
        S.conditional_affinities(torch.zeros(5, 257), torch.zeros(5, 257, dtype=torch.int64), 5.0)
    with pytest.raises(ValueError, match="prepare"):
        S.TSNE().step()


def test_evaluate_embedding_is_eval_mode_only_and_checks_its_arguments():
    x, y = torch.zeros(2, 3, 32, 32), torch.zeros(2, dtype=torch.int64)
    vae = S.VariationalAutoEncoder("wideresnet-10-1", num_input_channels=3, img_size=(32, 32), data_parallel=False,
                                   continuous_latent_dim=128, disc_latent_dim=10, small_input=True, compute_dtype="fp32")
    smooth = S.SmoothVAE((SO.KINDS["svhn"]["in_ch"], 32, 32), {"cont": 32, "disc": [10]}, compute_dtype="fp32")
    for m in (vae, smooth):
        m.train()
        with pytest.raises(NotImplementedError, match="eval mode only"):
            S.evaluate_embedding(m, [(x, y)])
        m.eval()
        with pytest.raises(L.ShotVaeHipError, match="MI355X"):
            S.evaluate_embedding(m, [(x, y)])
        with pytest.raises(ValueError, match="empty"):
            S.evaluate_embedding(m, [])
        with pytest.raises(ValueError, match=r"\(image, label\)"):
            S.evaluate_embedding(m, [x])
        with pytest.raises(ValueError, match="cosine"):
            S.evaluate_embedding(m, [(x, y)], metric="cosine")
        assert not m.training
    with pytest.raises(TypeError, match="VariationalAutoEncoder or a SmoothVAE"):
        S.evaluate_embedding(torch.nn.Linear(2, 2), [(x, y)])


# ================================================================================================ the outcome conditions of the GPU test
@pytest.mark.parametrize("n,classes,dim,k,perplexity", [(150, 3, 8, 30, 10.0), (130, 5, 16, 15, 5.0)])
def test_outcome_conditions_hold_for_the_restatement(n, classes, dim, k, perplexity):
    """the two conditions tests/test_tsne_gpu.py asserts of the device run hold for the float64 restatement from the PCA start"""
    P, y0, which = R.outcome_case(n, classes, dim, k, perplexity)
    y, kls = R.run(P, y0, 300, 100, 12.0, max(n / 12.0 / 4.0, 50.0))
    ratio, hit = R.kl(P, y) / kls[0], R.one_nn_hit(y, which)
    print("FIG outcome %s ratio %.3f hit %.3f" % ((n, classes, dim, k, perplexity), ratio, hit))
    assert ratio <= 0.5 and hit >= 0.95


def test_embedding_plot_scatter():
    from tools.embedding_plot import PALETTE, scatter
    y = np.array([[0.0, 0.0], [10.0, 0.0], [10.0, 5.0], [5.0, 2.5]])
    img = scatter(y, [0, 1, 12, -1], size=64, dot=3, margin=4)
    assert img.shape == (64, 64, 3) and img.dtype == np.uint8
    colours = {tuple(c) for c in img.reshape(-1, 3)}
    assert colours == {(255, 255, 255), tuple(PALETTE[0]), tuple(PALETTE[1]), tuple(PALETTE[2]), (0, 0, 0)}
    assert (img != 255).any(axis=2).sum() == 4 * 9, "four dots of 3 x 3, none clipped, none overlapping"
    xs = np.nonzero((img == PALETTE[1]).all(axis=2))[1]
    assert xs.max() == 64 - 4 - 1 and np.nonzero((img == PALETTE[0]).all(axis=2))[1].min() == 4, "one scale for both axes, inside the margin"
