"""Diagonal Gaussian mixtures without a GPU: the float64 restatement of tests/_gmm_ref.py pinned to scikit-learn, its identities, the
sampler's stream in numpy, the argument refusals of the five sv_gmm_* entry points (they validate before any HIP call) and the host
logic of shot_vae_amd.mixture."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import shot_vae_amd as S
from shot_vae_amd import _lib as L
from shot_vae_amd import mixture as MX
from tests import _gmm_ref as R

SV_E_ARG, SV_E_SHAPE = -1, -2


def start(x, k, seed):
    """a start from k rows of x: (weights, means, variances)"""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.5, 1.5, k)
    return w / w.sum(), x[rng.choice(len(x), k, replace=False)] + 0.1, rng.uniform(0.5, 2.0, (k, x.shape[1]))


# ================================================================================================ against scikit-learn
def test_one_restated_em_step_is_scikit_learns():
    sk = pytest.importorskip("sklearn.mixture")
    x, _, _ = R.blobs(150, 3, 5, 8101)
    w, m, v = start(x, 3, 8102)
    gm = sk.GaussianMixture(3, covariance_type="diag", weights_init=w, means_init=m, precisions_init=1.0 / v, max_iter=1, tol=0.0,
                            reg_covar=1e-6)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gm.fit(x)
    lw, mean, var, bound = R.em_step(x, np.log(w), m, v, 1e-6)
    errs = (np.abs(np.exp(lw) - gm.weights_).max(), np.abs(mean - gm.means_).max(), np.abs(var - gm.covariances_).max(),
            abs(bound - gm.lower_bound_))
    print("FIG one EM step against scikit-learn: weights %.1e means %.1e covariances %.1e bound %.1e" % errs)
    assert max(errs) <= 1e-12


def test_restatement_against_scikit_learns_building_blocks():
    gmod = pytest.importorskip("sklearn.mixture._gaussian_mixture")
    x, _, _ = R.blobs(90, 4, 6, 8103)
    w, m, v = start(x, 4, 8104)
    logp = gmod._estimate_log_gaussian_prob(x, m, 1.0 / np.sqrt(v), "diag") + np.log(w)
    assert np.abs(R.pair_values(x, np.log(w), m, v) - logp).max() <= 1e-11
    lse, assign, resp = R.estep(x, np.log(w), m, v)
    nk, means, cov = gmod._estimate_gaussian_parameters(x, resp, 1e-6, "diag")
    rk, _, rm, rv = R.mstep(x, resp, 1e-6)
    assert np.abs(rk - nk).max() <= 1e-12 and np.abs(rm - means).max() <= 1e-12 and np.abs(rv - cov).max() <= 1e-12
    assert np.array_equal(assign, logp.argmax(axis=1))


def test_bic_and_aic_are_scikit_learns():
    sk = pytest.importorskip("sklearn.mixture")
    x, _, _ = R.blobs(120, 3, 4, 8105)
    gm = sk.GaussianMixture(3, covariance_type="diag", random_state=0).fit(x)
    lw, m, v = np.log(gm.weights_), gm.means_, gm.covariances_
    total = R.estep(x, lw, m, v)[0].sum()
    npar = MX.n_parameters(3, 4)
    assert npar == R.n_parameters(3, 4) == gm._n_parameters() == 3 - 1 + 2 * 3 * 4
    assert abs(-2.0 * total + npar * math.log(len(x)) - gm.bic(x)) <= 1e-9 * abs(gm.bic(x))
    assert abs(-2.0 * total + 2.0 * npar - gm.aic(x)) <= 1e-9 * abs(gm.aic(x))


# ================================================================================================ identities
def test_one_component_is_the_sample_mean_and_the_biased_variance():
    x = np.random.default_rng(8106).normal(1.0, 2.0, (50, 3))
    lw, m, v, _ = R.em_step(x, np.zeros(1), np.zeros((1, 3)), np.ones((1, 3)), 1e-3)
    assert abs(lw[0]) <= 1e-15 and np.abs(m[0] - x.mean(axis=0)).max() <= 1e-13
    assert np.abs(v[0] - (x.var(axis=0) + 1e-3)).max() <= 1e-12


def test_responsibilities_sum_to_one_and_rules_of_special_rows():
    x, _, _ = R.blobs(40, 3, 4, 8107)
    lw, m, v = R.model(3, 4, 8108)
    lse, assign, resp = R.estep(x, lw, m, v)
    assert np.abs(resp.sum(axis=1) - 1.0).max() <= 1e-14 and np.isfinite(lse).all()
    x[3, 1], x[5, 0] = np.nan, np.inf
    lw[1] = -np.inf                                           # a component of weight 0 never wins and makes no NaN
    lse, assign, resp = R.estep(x, lw, m, v)
    assert np.isnan(lse[[3, 5]]).all() and (assign[[3, 5]] == -1).all() and np.isnan(resp[[3, 5]]).all()
    ok = np.ones(40, bool)
    ok[[3, 5]] = False
    assert np.isfinite(lse[ok]).all() and (resp[ok][:, 1] == 0).all() and (assign[ok] != 1).all()
    x[7] = 1e4                                                # a far outlier: finite, the responsibilities still sum to 1
    lse, _, resp = R.estep(x, lw, m, v)
    assert np.isfinite(lse[7]) and abs(resp[7].sum() - 1.0) <= 1e-12


def test_the_bound_never_decreases_over_20_restated_iterations():
    x, _, _ = R.blobs(200, 3, 4, 8109, spread=1.5)
    w, m, v = start(x, 3, 8110)
    lw, bounds = np.log(w), []
    for _ in range(20):
        lw, m, v, b = R.em_step(x, lw, m, v, 1e-6)
        bounds.append(b)
    assert all(b1 >= b0 - 1e-12 for b0, b1 in zip(bounds, bounds[1:])) and bounds[-1] > bounds[0]


def test_merging_partial_states_is_exact_in_the_restatement():
    """integer rows and dyadic responsibilities: every sum is exact, so any P and any cut give the same merged state -- and the states of
    the restatement's M-step are scikit-learn's"""
    rng = np.random.default_rng(8111)
    x = np.floor(rng.uniform(-4, 5, (300, 3)))
    r = rng.integers(0, 5, (300, 2)) / 4.0
    lse = rng.integers(-8, 8, 300) / 2.0
    lse[[5, 70]] = np.nan
    one = R.merge(R.accum(x, r, lse, 1)[0])
    for P in (2, 3, 5):
        sums, counts = R.accum(x, r, lse, P)
        assert np.array_equal(R.merge(sums), one) and counts.sum(axis=0).tolist() == [298, 2]
        a, ca = R.accum(x[:64 * P], r[:64 * P], lse[:64 * P], P)
        b, cb = R.accum(x[64 * P:], r[64 * P:], lse[64 * P:], P, a, ca)
        assert np.array_equal(b, sums) and np.array_equal(cb, counts)
    ok = np.isfinite(lse)
    lw, m, v, stats = R.finish(R.accum(x, r, lse, 3)[0], R.accum(x, r, lse, 3)[1], 2, 3, 1e-6, np.zeros(2), np.zeros((2, 3)), np.ones((2, 3)))
    nk, lw2, m2, v2 = R.mstep(x[ok], r[ok], 1e-6)
    assert np.abs(m - m2).max() <= 1e-13 and np.abs(v - v2).max() <= 1e-12 and np.abs(lw - lw2).max() <= 1e-14
    assert stats[1] == 298 and stats[2] == 2 and abs(stats[0] - lse[ok].mean()) <= 1e-13 and stats[3] == v.min()


def test_an_empty_component_keeps_its_parameters_in_the_restatement():
    x = np.arange(12.0).reshape(6, 2)
    r = np.stack([np.ones(6), np.zeros(6)], axis=1)
    sums, counts = R.accum(x, r, np.zeros(6), 1)
    lw, m, v, stats = R.finish(sums, counts, 2, 2, 0.0, np.zeros(2), np.full((2, 2), 7.0), np.full((2, 2), 3.0))
    assert lw[1] == -np.inf and abs(lw[0]) <= 1e-15 and (m[1] == 7.0).all() and (v[1] == 3.0).all()
    assert np.abs(m[0] - x.mean(axis=0)).max() <= 1e-14 and stats[3] == v[0].min()


# ================================================================================================ the sampler's stream
def test_the_tag_differs_from_the_three_existing_streams():
    tags = R.all_tags()
    assert set(tags) >= {"SV_LATENT_PHILOX_TAG", "SV_SCORE_PHILOX_TAG", "SV_GMM_PHILOX_TAG"}
    assert len(set(tags.values())) == len(tags) and 0 not in tags.values()          # (0: the dropout masks' fourth counter word)
    n = R.sample_normals(5, 10, 4, 9)
    for name, tag in tags.items():
        if name != "SV_GMM_PHILOX_TAG":
            assert not np.array_equal(R.sample_normals(5, 10, 4, 9, tag=tag), n)
    from tests.test_infer_cpu import latent_normals
    assert np.array_equal(R.sample_normals(5, 10, 4, 9, tag=tags["SV_LATENT_PHILOX_TAG"]), latent_normals(5, 10, 4, 9))


def test_the_stream_is_split_independent_and_standard_normal():
    n = R.sample_normals(77, 0, 4096, 6)
    assert np.array_equal(n[100:300], R.sample_normals(77, 100, 200, 6))
    assert abs(n.mean()) < 0.03 and abs(n.var() - 1.0) < 0.05
    u = R.sample_uniform(77, 0, 4096)
    assert np.array_equal(u[100:300], R.sample_uniform(77, 100, 200)) and (u >= 0).all() and (u < 1).all()
    assert abs(u.mean() - 0.5) < 0.02
    assert np.array_equal(R.sample_normals(77, 2 ** 33, 2, 5)[1], R.sample_normals(77, 2 ** 33 + 1, 1, 5)[0])


def test_component_choice_on_and_beside_a_cdf_edge():
    log = lambda w: np.log(np.maximum(w, 1e-300)) + np.where(np.asarray(w) > 0, 0.0, -np.inf)          # noqa: E731
    _, _, cdf = R.prepare(log([0.25, 0.0, 0.5, 0.25]), np.zeros((4, 1)), np.ones((4, 1)))
    assert cdf.tolist() == [0.25, 0.25, 0.75, 1.0]
    below, above = np.nextafter(0.25, 0.0), np.nextafter(0.25, 1.0)
    assert R.choose(cdf, np.array([0.0, below, 0.25, above, 0.75, 1.0 - 2.0 ** -24])).tolist() == [0, 0, 2, 2, 3, 3]
    # the zero-weight component is never the first: over every u the generator can give in a block of them
    u = np.arange(0, 2 ** 24, 4099) * 2.0 ** -24
    assert 1 not in R.choose(cdf, u)
    # a trailing component of weight 0: the last POSITIVE one carries the exact 1
    _, _, cdf = R.prepare(log([0.3, 0.7, 0.0]), np.zeros((3, 1)), np.ones((3, 1)))
    assert cdf[1] == 1.0 and 2 not in R.choose(cdf, u)


# ================================================================================================ the entry points' refusals
P4 = C.c_void_p(4096)               # never dereferenced: nothing is launched


def _prepare(**kw):
    a = dict(logw=P4, mean=P4, var=P4, K=3, D=4, ivar=P4, cst=P4, cdf=P4)
    a.update(kw)
    return L.lib().sv_gmm_prepare(a["logw"], a["mean"], a["var"], a["K"], a["D"], a["ivar"], a["cst"], a["cdf"], None)


def _estep(**kw):
    a = dict(x=P4, N=5, ivar=P4, mean=P4, cst=P4, K=3, D=4, lse=P4, assign=None, resp=None)
    a.update(kw)
    return L.lib().sv_gmm_estep(a["x"], a["N"], a["ivar"], a["mean"], a["cst"], a["K"], a["D"], a["lse"], a["assign"], a["resp"], None)


def _accum(**kw):
    a = dict(x=P4, lse=P4, N=5, ivar=P4, mean=P4, cst=P4, K=3, D=4, sums=P4, counts=P4, P=2, init=1)
    a.update(kw)
    return L.lib().sv_gmm_accum(a["x"], a["lse"], a["N"], a["ivar"], a["mean"], a["cst"], a["K"], a["D"], a["sums"], a["counts"], a["P"],
                                a["init"], None)


def _finish(**kw):
    a = dict(sums=P4, counts=P4, P=2, K=3, D=4, reg=1e-6, logw=P4, mean=P4, var=P4, ivar=P4, cst=P4, cdf=P4, stats=P4)
    a.update(kw)
    return L.lib().sv_gmm_finish(a["sums"], a["counts"], a["P"], a["K"], a["D"], a["reg"], a["logw"], a["mean"], a["var"], a["ivar"],
                                 a["cst"], a["cdf"], a["stats"], None)


def _sample(**kw):
    a = dict(mean=P4, var=P4, cdf=P4, K=3, D=4, key=P4, row0=0, B=2, z=P4, comp=None)
    a.update(kw)
    return L.lib().sv_gmm_sample(a["mean"], a["var"], a["cdf"], a["K"], a["D"], a["key"], a["row0"], a["B"], a["z"], a["comp"], None)


REFUSALS = [
    (_prepare, "sv_gmm_prepare", [(dict(logw=None), SV_E_ARG, b"NULL"), (dict(var=None), SV_E_ARG, b"NULL"), (dict(cdf=None), SV_E_ARG, b"NULL"),
                                  (dict(ivar=None), SV_E_ARG, b"NULL"), (dict(K=0), SV_E_ARG, b"size"), (dict(D=-1), SV_E_ARG, b"size")]),
    (_estep, "sv_gmm_estep", [(dict(x=None), SV_E_ARG, b"NULL"), (dict(cst=None), SV_E_ARG, b"NULL"), (dict(lse=None), SV_E_ARG, b"NULL"),
                              (dict(N=0), SV_E_ARG, b"size"), (dict(K=0), SV_E_ARG, b"size"), (dict(D=0), SV_E_ARG, b"size")]),
    (_accum, "sv_gmm_accum", [(dict(x=None), SV_E_ARG, b"NULL"), (dict(lse=None), SV_E_ARG, b"NULL"), (dict(mean=None), SV_E_ARG, b"NULL"),
                              (dict(sums=None), SV_E_ARG, b"NULL"), (dict(counts=None), SV_E_ARG, b"NULL"), (dict(N=0), SV_E_ARG, b"size"),
                              (dict(P=0), SV_E_ARG, b"P=0"), (dict(P=65), SV_E_ARG, b"P=65"), (dict(D=(1 << 20) + 1), SV_E_SHAPE, b"2^20"),
                              (dict(K=1 << 20, D=1 << 12), SV_E_SHAPE, b"31 bits")]),
    (_finish, "sv_gmm_finish", [(dict(sums=None), SV_E_ARG, b"NULL"), (dict(counts=None), SV_E_ARG, b"NULL"), (dict(logw=None), SV_E_ARG, b"NULL"),
                                (dict(cst=None), SV_E_ARG, b"NULL"), (dict(stats=None), SV_E_ARG, b"NULL"), (dict(K=0), SV_E_ARG, b"size"),
                                (dict(P=0), SV_E_ARG, b"P=0"), (dict(P=65), SV_E_ARG, b"P=65"), (dict(reg=-1e-9), SV_E_ARG, b"reg_covar"),
                                (dict(reg=float("nan")), SV_E_ARG, b"reg_covar"), (dict(reg=float("inf")), SV_E_ARG, b"reg_covar"),
                                (dict(K=1 << 20, D=1 << 12), SV_E_SHAPE, b"31 bits")]),
    (_sample, "sv_gmm_sample", [(dict(mean=None), SV_E_ARG, b"NULL"), (dict(cdf=None), SV_E_ARG, b"NULL"), (dict(key=None), SV_E_ARG, b"key"),
                                (dict(z=None), SV_E_ARG, b"NULL"), (dict(B=0), SV_E_ARG, b"size"), (dict(K=0), SV_E_ARG, b"size"),
                                (dict(row0=-1), SV_E_ARG, b"row0"), (dict(D=(1 << 30) + 1), SV_E_SHAPE, b"2^30")]),
]


@pytest.mark.parametrize("fn,name,cases", REFUSALS, ids=[r[1] for r in REFUSALS])
def test_entry_points_refuse_bad_arguments_before_any_launch(fn, name, cases):
    for kw, code, word in cases:
        assert fn(**kw) == code, (name, kw)
        err = L.lib().sv_last_error()
        assert word in err and name.encode() in err, (kw, err)


def test_entry_points_are_bound_and_exported():
    for name in ("sv_gmm_prepare", "sv_gmm_estep", "sv_gmm_accum", "sv_gmm_finish", "sv_gmm_sample"):
        assert name in L.EXPORTS and hasattr(L.lib(), name)
    assert L.lib().sv_version() == L.ABI_VERSION == 8
    for name in ("GaussianMixture", "evaluate_mixture", "generate_from_mixture"):
        assert getattr(S, name) is getattr(MX, name)


# ================================================================================================ host logic
def test_parameter_count_and_partials_are_functions_of_the_shapes():
    assert MX.n_parameters(1, 1) == 2 and MX.n_parameters(10, 128) == 9 + 2560
    for k, d, n in ((10, 128, 50000), (100, 128, 50000), (3, 5, 200), (1000, 512, 10 ** 6)):
        p = MX._partials(k, d, n)
        blocks = (1 if k <= 16 else -(-k // 64)) * -(-d // 32)
        assert 1 <= p <= 64 and p <= -(-n // 64) and (p == 1 or p * blocks <= 512) and p == MX._partials(k, d, n)
    assert MX._partials(10, 128, 50000) == 64 and MX._partials(3, 5, 100) == 2


def scripted(bounds, **kw):
    """_em_loop over a scripted sequence of bounds -> (iterations, converged, the reads it made)"""
    reads, it = [], iter(bounds)
    def read(previous, current):
        reads.append((previous, current))
        return (-math.inf if previous is None else previous), current
    n, conv, last = MX._em_loop(lambda: next(it), read, **kw)
    return n, conv, last, reads


def test_fit_stops_by_scikit_learns_rule_on_a_scripted_sequence():
    seq = [-10.0, -5.0, -4.0, -3.9995, -3.9994, -3.0]
    n, conv, last, reads = scripted(seq, max_iter=6, tol=1e-3, check_every=1)
    assert (n, conv, last) == (4, True, -3.9995) and len(reads) == 4 and reads[0] == (None, -10.0)
    n, conv, last, reads = scripted(seq, max_iter=6, tol=1e-3, check_every=2)          # iteration 4 is a checked one
    assert (n, conv, last) == (4, True, -3.9995) and reads == [(-10.0, -5.0), (-4.0, -3.9995)]
    n, conv, last, reads = scripted(seq, max_iter=6, tol=1e-3, check_every=3)          # 3 and 6 are checked: 5 -> 6 moved by 1
    assert (n, conv) == (6, False) and len(reads) == 2
    n, conv, last, reads = scripted(seq, max_iter=5, tol=1e-3, check_every=3)          # the last iteration is always checked
    assert (n, conv, last) == (5, True, -3.9994) and reads == [(-5.0, -4.0), (-3.9995, -3.9994)]
    n, conv, last, reads = scripted(seq, max_iter=6, tol=None, check_every=1)          # never with tol=None
    assert (n, conv, last) == (6, False, -3.0) and reads == []
    n, conv, last, reads = scripted([-1.0], max_iter=1, tol=1e-3, check_every=1)       # the first bound is compared with -inf
    assert (n, conv) == (1, False)
    n, conv, _, _ = scripted([-2.0, -2.0005], max_iter=2, tol=1e-3, check_every=1)     # |change|, as scikit-learn
    assert (n, conv) == (2, True)


def test_state_dict_round_trip_on_the_host():
    gm = S.GaussianMixture(3, 4, reg_covar=1e-4)
    with pytest.raises(ValueError, match="no parameters"):
        gm.state_dict()
    lw, m, v = (torch.from_numpy(a).float() for a in R.model(3, 4, 8112))
    gm.load_state_dict(dict(k=3, dim=4, reg_covar=1e-5, logw=lw, mean=m, var=v, converged=True, n_iter=7))
    sd = gm.state_dict()
    other = S.GaussianMixture(3, 4).load_state_dict(sd)
    for name in ("logw", "mean", "var"):
        assert torch.equal(getattr(other, name), getattr(gm, name)) and getattr(other, name) is not sd[name]
    assert other.reg_covar == 1e-5 and other.converged_ is True and other.n_iter_ == 7
    assert torch.allclose(other.weights.sum(), torch.tensor(1.0), atol=1e-6)
    with pytest.raises(ValueError, match="3 x 4"):
        S.GaussianMixture(2, 4).load_state_dict(sd)
    with pytest.raises(ValueError, match="mean"):
        S.GaussianMixture(3, 4).load_state_dict(dict(sd, mean=m[:2]))
    # a mixture that is still on the host is refused at its first use
    for call in (lambda: other.score_samples(torch.zeros(2, 4)), lambda: other.sample(2, 0)):
        with pytest.raises(L.ShotVaeHipError, match="MI355X"):
            call()


def test_python_layer_refuses_bad_arguments():
    for k, d in ((0, 4), (2, 0), (2, (1 << 20) + 1), (1 << 14, 1 << 17)):
        with pytest.raises(ValueError):
            S.GaussianMixture(k, d)
    for reg in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="reg_covar"):
            S.GaussianMixture(2, 4, reg_covar=reg)
    with pytest.raises(ValueError, match="init must be"):
        S.GaussianMixture(2, 4, init="k-means++")
    gm = S.GaussianMixture(2, 4)
    with pytest.raises(ValueError, match="no parameters"):
        gm.sample(3, 0)
    with pytest.raises(ValueError, match=">= 1"):
        gm.fit(torch.zeros(6, 4), max_iter=0)
    with pytest.raises(ValueError, match="tol"):
        gm.fit(torch.zeros(6, 4), tol=-1.0)
    with pytest.raises(TypeError):
        S.evaluate_mixture(object(), [])
    with pytest.raises(TypeError):
        S.generate_from_mixture(object(), gm, torch.zeros(2, dtype=torch.int64), 0)


def test_python_layer_checks_shapes_before_it_asks_for_the_device():
    x = torch.zeros(6, 4)
    gm = S.GaussianMixture(7, 4)
    with pytest.raises(ValueError, match="k > N"):
        gm.fit(x)
    with pytest.raises(ValueError, match="columns"):
        S.GaussianMixture(2, 5).fit(x)
    with pytest.raises(ValueError, match="matrix"):
        S.GaussianMixture(2, 4).fit(x.view(-1))
    gm = S.GaussianMixture(2, 4)
    with pytest.raises(ValueError, match="weights"):
        gm.set_parameters(torch.ones(3), torch.zeros(2, 4), torch.ones(2, 4))
    with pytest.raises(ValueError, match="weights"):
        gm.set_parameters(torch.ones(2), torch.zeros(2, 5), torch.ones(2, 4))
    # ... and then the no-CPU rule
    with pytest.raises(L.ShotVaeHipError, match="MI355X"):
        gm.set_parameters(torch.ones(2) / 2, torch.zeros(2, 4), torch.ones(2, 4))
    for call in (lambda: gm.fit(x), lambda: gm.reset(x)):
        with pytest.raises(L.ShotVaeHipError, match="MI355X"):
            call()
    gm.load_state_dict(dict(k=2, dim=4, logw=torch.zeros(2), mean=torch.zeros(2, 4), var=torch.ones(2, 4)))
    for call in (lambda: gm.step(x), lambda: gm.predict(x), lambda: gm.predict_proba(x), lambda: gm.score(x), lambda: gm.bic(x)):
        with pytest.raises(L.ShotVaeHipError, match="MI355X"):
            call()
    with pytest.raises(ValueError, match="columns"):
        gm.score_samples(torch.zeros(6, 5))


def test_the_joins_refuse_a_mixture_out_of_place():
    """the new arguments of evaluate_generation / evaluate_detection are checked before anything runs"""
    from shot_vae_amd import calibration, quality
    assert "mixture" in calibration.SCORES
    import inspect
    assert inspect.signature(quality.evaluate_generation).parameters["mixture"].default is None
    assert inspect.signature(calibration.evaluate_detection).parameters["mixture"].default is None
