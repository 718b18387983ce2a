"""Generation-quality metrics without a GPU: the float64 restatement of tests/_quality_ref.py against closed forms (the Frechet distance
of commuting covariances, numpy.cov, scipy's sqrtm where it is installed; counts and metrics of sets whose answer is known), the
argument refusals of sv_ball_scan through the library, and the Python layer's errors (shot_vae_amd/quality.py)."""
import numpy as np
import pytest
import torch

import shot_vae_amd as S
from shot_vae_amd import _lib as L
from shot_vae_amd import quality as QL
from oracle import smooth_oracle as SO
from tests import _knn_ref as R
from tests import _quality_ref as QR

SV_E_ARG, SV_E_SHAPE = -1, -2    # include/shotvae_hip.h
PTR = 4096                       # never dereferenced: a refused call launches nothing
FRECHETS = [QR.frechet, QL.frechet_from_moments]          # the restatement and the package's host formula: the same checks


def spd(D, seed, scale=1.0):
    rng = np.random.RandomState(seed)
    a = rng.randn(3 * D, D) * scale
    return rng.randn(D), a.T @ a / (3 * D - 1)


# ================================================================================================ the Frechet formula
@pytest.mark.parametrize("fn", FRECHETS)
def test_frechet_equals_the_closed_form_for_commuting_covariances(fn):
    """diagonal covariances: tr sqrt(S1^1/2 S2 S1^1/2) = sum sqrt(a_i b_i), so d = |dm|^2 + sum (sqrt a_i - sqrt b_i)^2; and the same
    pair rotated by one orthogonal matrix (still commuting, no longer diagonal)"""
    rng = np.random.RandomState(4201)
    for D in (1, 7, 40):
        a, b = rng.uniform(0.1, 3.0, D), rng.uniform(0.1, 3.0, D)
        m1, m2 = rng.randn(D), rng.randn(D)
        want = float(np.sum((m1 - m2) ** 2) + np.sum((np.sqrt(a) - np.sqrt(b)) ** 2))
        assert abs(fn(m1, np.diag(a), m2, np.diag(b)) - want) <= 1e-12 * (a.sum() + b.sum())
        q = np.linalg.qr(rng.randn(D, D))[0]
        assert abs(fn(m1, q @ np.diag(a) @ q.T, m2, q @ np.diag(b) @ q.T) - want) <= 1e-11 * (a.sum() + b.sum())


@pytest.mark.parametrize("fn", FRECHETS)
def test_frechet_is_symmetric_and_zero_on_identical_sets(fn):
    for D, seed in ((7, 4203), (40, 4205)):
        (m1, s1), (m2, s2) = spd(D, seed), spd(D, seed + 1, 1.7)
        tr = np.trace(s1) + np.trace(s2)
        assert abs(fn(m1, s1, m2, s2) - fn(m2, s2, m1, s1)) <= 1e-12 * tr
        assert fn(m1, s1, m2, s2) > 1e-3 * tr
        assert abs(fn(m1, s1, m1, s1)) <= 1e-12 * 2.0 * np.trace(s1)
    # rows, fewer than dimensions: a rank-deficient covariance against itself
    x = np.random.RandomState(4207).randn(20, 40)
    assert abs(QR.frechet_of_rows(x, x)) <= 1e-12 * 2.0 * np.trace(QR.moments(x)[1])


@pytest.mark.parametrize("fn", FRECHETS)
def test_frechet_equals_the_sqrtm_form(fn):
    """tr sqrt(S1^1/2 S2 S1^1/2) = tr sqrtm(S1 S2): the form the FID implementations evaluate"""
    linalg = pytest.importorskip("scipy.linalg")
    for D, seed in ((7, 4209), (40, 4211)):
        (m1, s1), (m2, s2) = spd(D, seed), spd(D, seed + 1, 0.6)
        root = linalg.sqrtm(s1 @ s2)
        want = float(np.sum((m1 - m2) ** 2) + np.trace(s1) + np.trace(s2) - 2.0 * np.trace(root).real)
        assert abs(fn(m1, s1, m2, s2) - want) <= 1e-9 * (np.trace(s1) + np.trace(s2))


def test_both_frechet_formulas_agree_on_rank_deficient_moments():
    a, b = np.random.RandomState(4213).randn(20, 40), np.random.RandomState(4215).randn(30, 40) + 0.3
    ma, mb = QR.moments(a), QR.moments(b)
    tr = np.trace(ma[1]) + np.trace(mb[1])
    assert abs(QR.frechet(*ma, *mb) - QL.frechet_from_moments(*ma, *mb)) <= 1e-12 * tr


def test_shifted_moments_equal_numpy_cov_far_from_the_origin():
    x = 1.0e4 + np.random.RandomState(4217).randn(300, 9)
    for cuts in ([300], [1, 300], [64, 128, 300]):
        edges = [0] + cuts
        mean, cov = QR.shifted_moments([x[a:b] for a, b in zip(edges[:-1], edges[1:])])
        assert np.abs(mean - x.mean(axis=0)).max() <= 1e-11 * 1.0e4
        assert np.abs(cov - np.cov(x, rowvar=False)).max() <= 1e-11
    m2, c2 = QR.moments(x)
    assert np.abs(c2 - np.cov(x, rowvar=False)).max() <= 1e-12 and np.abs(m2 - x.mean(axis=0)).max() <= 1e-11 * 1.0e4


# ================================================================================================ counts and metrics
@pytest.mark.parametrize("metric", ("euclid", "w2"))
def test_identical_sets_are_precise_and_covered(metric):
    mu, ls = R.posterior(40, 7, 4221)
    res = QR.metrics(metric, mu, ls, mu, ls, 3)
    assert res["precision"] == res["recall"] == res["coverage"] == 1.0 and res["density"] >= 1.0
    assert res["n_real"] == res["n_fake"] == 40


@pytest.mark.parametrize("metric", ("euclid", "w2"))
def test_clusters_farther_apart_than_any_radius_share_nothing(metric):
    mu, ls = R.posterior(40, 7, 4223)
    far = mu + 100.0
    assert QR.radii(metric, mu, ls, 3).max() < 100.0
    res = QR.metrics(metric, mu, ls, far, ls, 3)
    assert res["precision"] == res["recall"] == res["coverage"] == res["density"] == 0.0


def test_radius_rules():
    mu = np.array([[0.0], [0.0], [1.0], [3.0], [np.nan], [np.inf]])        # rows 0 and 1 coincide
    with np.errstate(invalid="ignore", over="ignore"):
        dist = R.distances("euclid", mu, None, mu[:4], None)                 # [6, 4]
    for r, want in ((np.nan, 0), (-1.0, 0), (np.inf, 4), (0.0, None)):
        m = QR.inside(dist, np.full(4, r))
        if want is not None:
            assert m[:4].sum(axis=1).tolist() == [want] * 4
        assert not m[4:].any()                                               # a NaN and an infinite row are inside nothing
    m = QR.inside(dist, np.zeros(4))
    assert m[:4].astype(int).tolist() == [[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]
    # the boundary belongs to the ball: radius 1 around row 2 (value 1.0) holds rows 0 and 1 exactly
    assert QR.inside(dist, np.array([-1.0, -1.0, 1.0, -1.0]))[:, 2].tolist() == [True, True, True, False, False, False]
    # a NaN gallery row is a ball that holds nothing, even with radius +inf
    assert not QR.inside(R.distances("euclid", mu[:4], None, mu[4:5], None), np.array([np.inf])).any()


def test_self_exclusion_and_radii_are_leave_one_out():
    mu, ls = R.posterior(30, 5, 4225)
    dist = R.distances("euclid", mu, None, mu, None)
    r = QR.radii("euclid", mu, None, 1)
    assert (r > 0).all() and np.array_equal(r, np.sort(dist + np.diag(np.full(30, np.inf)), axis=1)[:, 0])
    with_self, without = QR.counts(dist, r)[0], QR.counts(dist, r, self0=0)[0]
    assert np.array_equal(with_self, without + 1)
    # self0 beyond the columns, and shifted into them
    assert np.array_equal(QR.counts(dist, r, self0=30)[0], with_self)
    q, g = QR.counts(dist[10:], r, self0=10)
    assert np.array_equal(q, without[10:]) and g.sum() == q.sum()


@pytest.mark.parametrize("cuts", [[130], [1, 65, 130], list(range(10, 131, 10))])
def test_counts_do_not_depend_on_the_cut(cuts):
    qm, ql = R.posterior(33, 7, 4227)
    gm, gl = R.posterior(130, 7, 4229)
    dist = R.distances("w2", qm, ql, gm, gl)
    r = QR.radii("w2", gm, gl, 3)
    q1, g1 = QR.counts(dist, r, self0=40)
    q2, g2 = np.zeros(33, np.int64), np.zeros(130, np.int64)
    edges = [0] + cuts
    for a, b in zip(edges[:-1], edges[1:]):
        q, g = QR.counts(dist[:, a:b], r[a:b], col0=a, self0=40)
        q2 += q
        g2[a:b] += g
    assert np.array_equal(q1, q2) and np.array_equal(g1, g2) and 0 < q1.sum() < 33 * 130
    qa, ga = QR.counts(dist[:1], r, self0=40)
    qb, gb = QR.counts(dist[1:], r, self0=41)
    assert np.array_equal(np.concatenate([qa, qb]), q1) and np.array_equal(ga + gb, g1)


# ================================================================================================ argument refusals
def _scan(**kw):
    a = dict(metric=L.DIST_EUCLID, q_mu=PTR, q_ls=None, Q=3, g_mu=PTR, g_ls=None, g_r=PTR, N=5, D=7, col0=0, self0=-1, P=2, q_count=PTR,
             g_count=PTR)
    a.update(kw)
    return L.lib().sv_ball_scan(a["metric"], a["q_mu"], a["q_ls"], a["Q"], a["g_mu"], a["g_ls"], a["g_r"], a["N"], a["D"], a["col0"],
                                a["self0"], a["P"], a["q_count"], a["g_count"], None)


W2 = dict(metric=L.DIST_W2, q_ls=PTR, g_ls=PTR)


@pytest.mark.parametrize("kw,code,word", [
    (dict(metric=-1), SV_E_ARG, b"metric"), (dict(metric=4), SV_E_ARG, b"metric"), (dict(metric=L.DIST_KL, q_ls=PTR, g_ls=PTR), SV_E_ARG, b"metric"),
    (dict(metric=L.DIST_COSINE), SV_E_ARG, b"metric"),
    (dict(q_mu=None), SV_E_ARG, b"NULL"), (dict(g_mu=None), SV_E_ARG, b"NULL"), (dict(g_r=None), SV_E_ARG, b"NULL"),
    (dict(W2, q_ls=None), SV_E_ARG, b"reads ls"), (dict(W2, g_ls=None), SV_E_ARG, b"reads ls"),
    (dict(q_count=None, g_count=None), SV_E_ARG, b"no output"),
    (dict(Q=0), SV_E_ARG, b"size"), (dict(N=0), SV_E_ARG, b"size"), (dict(D=0), SV_E_ARG, b"size"), (dict(Q=-3), SV_E_ARG, b"size"),
    (dict(N=-4), SV_E_ARG, b"size"), (dict(D=-1), SV_E_ARG, b"size"),
    (dict(col0=-1), SV_E_ARG, b"col0"), (dict(self0=-2), SV_E_ARG, b"self0"),
    (dict(P=0), SV_E_ARG, b"P=0"), (dict(P=65), SV_E_ARG, b"P=65"), (dict(P=-1), SV_E_ARG, b"P=-1"),
    (dict(col0=2 ** 63 - 10), SV_E_SHAPE, b"overflows"), (dict(self0=2 ** 63 - 10), SV_E_SHAPE, b"overflows")])
def test_ball_scan_refuses_bad_arguments_before_any_launch(kw, code, word):
    assert _scan(**kw) == code
    assert word in L.lib().sv_last_error() and b"sv_ball_scan" in L.lib().sv_last_error()


def test_refusals_leave_the_valid_forms_alone():
    """probed through a LATER refusal: ls may be NULL under the Euclidean metric, either counter may be NULL, P = 1 and P = 64 are
    valid, self0 = -1 and 0 are valid, W2 with both ls is valid"""
    for kw in (dict(), dict(q_count=None), dict(g_count=None), dict(P=1), dict(P=64), dict(self0=0), dict(W2), dict(q_ls=PTR, g_ls=PTR)):
        assert _scan(col0=2 ** 63 - 10, **kw) == SV_E_SHAPE and b"overflows" in L.lib().sv_last_error()


def test_entry_point_is_bound_and_exported():
    assert "sv_ball_scan" in L.EXPORTS and hasattr(L.lib(), "sv_ball_scan")
    assert L.lib().sv_version() == L.ABI_VERSION == 8
    for name in ("Manifold", "manifold_metrics", "FeatureMoments", "frechet_distance", "evaluate_generation"):
        assert getattr(S, name) is getattr(QL, name)


# ================================================================================================ the Python layer
def test_python_layer_refuses_cpu_tensors_and_bad_arguments():
    mu = torch.zeros(6, 8)
    man = S.Manifold(8)
    with pytest.raises(L.ShotVaeHipError, match="MI355X|no CPU fallback"):
        man.add(mu)
    assert len(man) == 0
    with pytest.raises(ValueError, match="fit"):                 # count before fit
        man.count(mu)
    with pytest.raises(ValueError, match="more than k"):         # k >= len (an empty set included)
        man.fit(1)
    for bad in (0, -1, 257):
        with pytest.raises(ValueError, match="k must be"):
            man.fit(bad)
    for metric in ("kl", "cosine"):
        with pytest.raises(ValueError, match="symmetric"):
            S.Manifold(8, metric)
        with pytest.raises(ValueError, match="symmetric"):
            S.manifold_metrics(mu, mu, metric=metric)
    with pytest.raises(ValueError, match="unknown metric"):
        S.Manifold(8, "manhattan")
    with pytest.raises(ValueError, match="dim must be >= 1"):
        S.Manifold(0)
    with pytest.raises(L.ShotVaeHipError, match="MI355X"):
        S.manifold_metrics(mu, mu)
    for a, b in ((mu, torch.zeros(6, 7)), (mu.view(-1), mu), (None, mu)):
        with pytest.raises(ValueError, match="matrices"):
            S.manifold_metrics(a, b)
    mom = S.FeatureMoments(8)
    with pytest.raises(L.ShotVaeHipError, match="MI355X"):
        mom.add(mu)
    for fn in (lambda: mom.add(None), lambda: mom.mean(), lambda: mom.cov(), lambda: S.FeatureMoments(0),
               lambda: S.frechet_distance(mom, mom)):
        with pytest.raises(ValueError):
            fn()
    with pytest.raises(TypeError, match="FeatureMoments"):
        S.frechet_distance(mom, (np.zeros(8), np.eye(8)))


def test_evaluate_generation_is_eval_mode_only_and_checks_its_arguments():
    x = torch.zeros(2, 3, 32, 32)
    vae = S.VariationalAutoEncoder("wideresnet-10-1", num_input_channels=3, img_size=(32, 32), data_parallel=False,
                                   continuous_latent_dim=128, disc_latent_dim=10, small_input=True, compute_dtype="fp32")
    smooth = S.SmoothVAE((SO.KINDS["svhn"]["in_ch"], 32, 32), {"cont": 32, "disc": [10]}, compute_dtype="fp32")
    for m in (vae, smooth):
        m.train()
        with pytest.raises(NotImplementedError, match="eval mode only"):
            S.evaluate_generation(m, [x])
        m.eval()
        with pytest.raises(L.ShotVaeHipError, match="MI355X"):
            S.evaluate_generation(m, [x], source="reconstruct")
        with pytest.raises(L.ShotVaeHipError, match="MI355X"):
            S.evaluate_generation(m, [(x, torch.zeros(2, dtype=torch.int64))])
        with pytest.raises(ValueError, match="empty"):
            S.evaluate_generation(m, [])
        for kw, word in ((dict(source="sample"), "source"), (dict(space="pixels"), "space"), (dict(metric="kl"), "symmetric"),
                         (dict(metric="cosine"), "symmetric"), (dict(k=0), "k must be"), (dict(k=257), "k must be"),
                         (dict(key=None), "key"), (dict(space="features", metric="w2"), "features")):
            with pytest.raises(ValueError, match=word):
                S.evaluate_generation(m, [x], **kw)
        assert not m.training
    with pytest.raises(ValueError, match="features"):
        S.evaluate_generation(smooth, [x], space="features")
    with pytest.raises(TypeError, match="VariationalAutoEncoder or a SmoothVAE"):
        S.evaluate_generation(torch.nn.Linear(2, 2), [x])
