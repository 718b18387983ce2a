"""The aggregate posterior without a GPU: the float64 restatement of tests/_aggpost_ref.py against torch.distributions.Normal.log_prob,
its identities (identical rows carry no information, D = 1, mi + marginal_kl = kl_c_mc, lpz - lqx = sv_latent_sweep's lw, partial states
merge exactly), the argument refusals of the four sv_aggpost_* entry points through the library, and the Python layer's errors."""
import math

import numpy as np
import pytest
import torch

import shot_vae_amd as S
from shot_vae_amd import _lib as L
from shot_vae_amd import aggregate as AG
from oracle import smooth_oracle as SO
from tests import _aggpost_ref as A
from tests import _score_ref as SR

SV_E_ARG, SV_E_SHAPE = -1, -2    # include/shotvae_hip.h
PTR = 4096                       # never dereferenced: a refused call launches nothing


def torch_logq(z, mu, ls):
    """(log q(z) [Q], log q(z_d) [Q, D]) of the uniform mixture, with torch.distributions in float64"""
    z, mu, ls = (torch.from_numpy(np.asarray(a, np.float64)) for a in (z, mu, ls))
    lp = torch.distributions.Normal(mu[None], torch.exp(ls)[None]).log_prob(z[:, None, :])           # [Q, N, D]
    n = math.log(mu.shape[0])
    return (torch.logsumexp(lp.sum(dim=2), dim=1) - n).numpy(), (torch.logsumexp(lp, dim=1) - n).numpy()


# ================================================================================================ the restatement
@pytest.mark.parametrize("recipe", A.RECIPES)
@pytest.mark.parametrize("N,D", [(1, 7), (3, 7), (3, 1), (130, 17)])
def test_float64_restatement_matches_torch_distributions(recipe, N, D):
    """one gallery row, a mixture of three, and a case with a ragged 16-block"""
    mu, ls = A.rows(recipe, N, D, 9811)
    z = A.queries(recipe, 9, D, 9813)
    lq, lqd = torch_logq(z, mu, ls)
    assert np.abs(A.log_density(z, mu, ls) - lq).max() <= 1e-11 * max(1.0, np.abs(lq).max())
    assert np.abs(A.log_density_dims(z, mu, ls) - lqd).max() <= 1e-11 * max(1.0, np.abs(lqd).max())
    if N == 1:
        want = torch.distributions.Normal(torch.from_numpy(mu), torch.exp(torch.from_numpy(ls))).log_prob(torch.from_numpy(z)[:, None, :])
        assert np.abs(A.pair_values(z, mu, ls) - want.sum(dim=2).numpy()).max() <= 1e-11 * D * 10


def test_sample_terms_match_torch_distributions_and_the_sweep():
    mu, ls = A.rows("spread", 11, 130, 9815)
    for key in (None, 12345):
        z, lqx, lpz = A.sample(mu, ls, key, 40, 3)
        tz, tm, ts = torch.from_numpy(z), torch.from_numpy(mu), torch.exp(torch.from_numpy(ls))
        assert np.abs(lqx - torch.distributions.Normal(tm, ts).log_prob(tz).sum(dim=1).numpy()).max() <= 1e-9
        assert np.abs(lpz - torch.distributions.Normal(0.0, 1.0).log_prob(tz).sum(dim=1).numpy()).max() <= 1e-9
        # lpz - lqx is the importance weight sv_latent_sweep writes for (key, row0, s): its S = 4 sweep's sample 3
        lw = SR.sweep_lw(key, 40, 11, 4, 130, mu, ls)[:, 3]
        assert np.abs((lpz - lqx) - lw).max() <= 1e-10
        assert np.array_equal(z, SR.sweep_z(key, 40, 11, 4, 130, mu, ls)[:, 3])
    assert np.array_equal(A.sample(mu, ls, None, 0, 0)[0], mu)


def test_identical_gallery_rows_carry_no_information():
    mu, ls = A.rows("spread", 1, 17, 9817)
    mu, ls = np.repeat(mu, 12, axis=0), np.repeat(ls, 12, axis=0)
    res = A.diagnostics(mu, ls, np.full((12, 4), 0.25), samples=2, key=5)
    assert abs(res["mi"]) <= 1e-12 and abs(res["mi_y"]) <= 1e-12 and abs(res["marginal_kl_y"]) <= 1e-12
    assert res["active_units"] == 0


def test_one_dimension_per_dimension_equals_joint():
    mu, ls = A.rows("overlap", 65, 1, 9819)
    z = A.queries("overlap", 9, 1, 9821)
    assert np.abs(A.log_density_dims(z, mu, ls)[:, 0] - A.log_density(z, mu, ls)).max() <= 1e-12
    res = A.diagnostics(mu, ls, np.full((65, 2), 0.5))
    assert abs(res["total_correlation"]) <= 1e-12 and abs(res["dimwise_kl"] - res["marginal_kl"]) <= 1e-12


@pytest.mark.parametrize("recipe", A.RECIPES)
def test_the_split_of_the_average_kl(recipe):
    mu, ls = A.rows(recipe, 40, 16, 9823)
    qy = np.abs(A.rows("spread", 40, 5, 9825)[0]) + 0.1
    qy /= qy.sum(axis=1, keepdims=True)
    res = A.diagnostics(mu, ls, qy, samples=3, key=9)
    assert abs(res["mi"] + res["marginal_kl"] - res["kl_c_mc"]) <= 1e-12 * max(1.0, abs(res["kl_c_mc"]))
    assert abs(res["total_correlation"] + res["dimwise_kl"] - res["marginal_kl"]) <= 1e-10
    assert res["mi"] <= res["log_n"] + 1e-12 and res["mi_y"] >= -1e-12 and res["mi_y"] <= math.log(5)
    assert res["dim_kl"].shape == (16,) and abs(res["dim_kl"].sum() - res["dimwise_kl"]) <= 1e-10
    # the Monte-Carlo KL estimates the analytic one: 120 draws of a 16-dimensional KL
    assert abs(res["kl_c_mc"] - res["kl_c"]) <= 0.25 * max(1.0, res["kl_c"])


@pytest.mark.parametrize("cuts", [[130], [1, 65, 130], list(range(10, 131, 10)), [0, 64, 64, 130]])
def test_partial_states_merge_to_the_single_state(cuts):
    mu, ls = A.rows("overlap", 130, 17, 9827)
    z = A.queries("overlap", 9, 17, 9829)
    v = A.pair_values(z, mu, ls)
    v[2, 5] = -np.inf
    one = A.finish(*(a[None] for a in A.state(v, 1)), 130)
    edges = [0] + cuts
    parts = [A.state(v[:, a:b], 1) for a, b in zip(edges[:-1], edges[1:])]
    got = A.finish(np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]), 130)
    assert np.abs(got - one).max() <= 1e-12
    # the rules: an empty row is -inf, a NaN stays, +inf stays
    m = np.array([[-np.inf, np.nan, np.inf, 0.0], [-np.inf, 1.0, 2.0, -np.inf]])
    s = np.array([[0.0, 0.0, 1.0, 2.0], [0.0, 1.0, 1.0, 0.0]])
    out = A.finish(m, s, 2)
    assert out[0] == -np.inf and np.isnan(out[1]) and out[2] == np.inf and out[3] == 0.0


def test_overlap_inputs_have_many_contributing_terms():
    for D in (1, 16, 17, 128, 130):
        mu, ls = A.rows("overlap", 130, D, 9801)
        assert A.min_ess(A.queries("overlap", 70, D, 9803), mu, ls) >= A.MIN_ESS, D
    mu, ls = A.rows("spread", 130, 128, 9801)
    assert A.min_ess(A.queries("spread", 70, 128, 9803), mu, ls) < 1.5


# ================================================================================================ argument refusals
def _sample(**kw):
    a = dict(mu=PTR, ls=PTR, key=PTR, row0=0, s=0, Q=3, D=7, z=PTR, lqx=PTR, lpz=PTR)
    a.update(kw)
    return L.lib().sv_aggpost_sample(a["mu"], a["ls"], a["key"], a["row0"], a["s"], a["Q"], a["D"], a["z"], a["lqx"], a["lpz"], None)


def _density(name, **kw):
    a = dict(z=PTR, Q=3, g_mu=PTR, g_ls=PTR, N=5, D=7, col0=0, self0=-1, m=PTR, s=PTR, P=2, init=1)
    a.update(kw)
    return getattr(L.lib(), name)(a["z"], a["Q"], a["g_mu"], a["g_ls"], a["N"], a["D"], a["col0"], a["self0"], a["m"], a["s"], a["P"],
                                  a["init"], None)


def _finish(**kw):
    a = dict(m=PTR, s=PTR, P=2, R=3, count=5, out=PTR)
    a.update(kw)
    return L.lib().sv_aggpost_finish(a["m"], a["s"], a["P"], a["R"], a["count"], a["out"], None)


@pytest.mark.parametrize("kw,code,word", [
    (dict(mu=None), SV_E_ARG, b"NULL"), (dict(ls=None), SV_E_ARG, b"NULL"), (dict(z=None), SV_E_ARG, b"NULL"),
    (dict(lqx=None), SV_E_ARG, b"NULL"), (dict(lpz=None), SV_E_ARG, b"NULL"), (dict(Q=0), SV_E_ARG, b"size"), (dict(D=0), SV_E_ARG, b"size"),
    (dict(Q=-2), SV_E_ARG, b"size"), (dict(row0=-1), SV_E_ARG, b"row0"), (dict(s=-1), SV_E_ARG, b"s=-1"),
    (dict(s=65536), SV_E_SHAPE, b"counter"), (dict(D=(1 << 18) + 1), SV_E_SHAPE, b"counter")])
def test_sample_refuses_bad_arguments_before_any_launch(kw, code, word):
    assert _sample(**kw) == code
    assert word in L.lib().sv_last_error() and b"sv_aggpost_sample" in L.lib().sv_last_error()


@pytest.mark.parametrize("name", ["sv_aggpost_scan", "sv_aggpost_dims"])
@pytest.mark.parametrize("kw,code,word", [
    (dict(z=None), SV_E_ARG, b"NULL"), (dict(g_mu=None), SV_E_ARG, b"NULL"), (dict(g_ls=None), SV_E_ARG, b"NULL"),
    (dict(m=None), SV_E_ARG, b"state"), (dict(s=None), SV_E_ARG, b"state"),
    (dict(Q=0), SV_E_ARG, b"size"), (dict(N=0), SV_E_ARG, b"size"), (dict(D=0), SV_E_ARG, b"size"), (dict(N=-4), SV_E_ARG, b"size"),
    (dict(P=0), SV_E_ARG, b"P=0"), (dict(P=65), SV_E_ARG, b"P=65"), (dict(P=-1), SV_E_ARG, b"P=-1"),
    (dict(col0=-1), SV_E_ARG, b"col0"), (dict(self0=-2), SV_E_ARG, b"self0"), (dict(col0=2 ** 63 - 10), SV_E_SHAPE, b"overflows")])
def test_density_passes_refuse_bad_arguments_before_any_launch(name, kw, code, word):
    assert _density(name, **kw) == code
    assert word in L.lib().sv_last_error() and name.encode() in L.lib().sv_last_error()


@pytest.mark.parametrize("kw,code,word", [
    (dict(m=None), SV_E_ARG, b"NULL"), (dict(s=None), SV_E_ARG, b"NULL"), (dict(out=None), SV_E_ARG, b"NULL"),
    (dict(P=0), SV_E_ARG, b"P=0"), (dict(P=65), SV_E_ARG, b"P=65"), (dict(R=0), SV_E_ARG, b"size"), (dict(R=-1), SV_E_ARG, b"size"),
    (dict(count=0), SV_E_ARG, b"count"), (dict(count=-3), SV_E_ARG, b"count")])
def test_finish_refuses_bad_arguments_before_any_launch(kw, code, word):
    assert _finish(**kw) == code
    assert word in L.lib().sv_last_error() and b"sv_aggpost_finish" in L.lib().sv_last_error()


def test_refusals_leave_the_valid_forms_alone():
    """probed through a LATER refusal: key may be NULL, P = 1 and P = 64 are valid, self0 = -1 and 0 are valid"""
    assert _sample(key=None, s=65536) == SV_E_SHAPE and b"counter" in L.lib().sv_last_error()
    for name in ("sv_aggpost_scan", "sv_aggpost_dims"):
        for kw in (dict(P=1), dict(P=64), dict(self0=0), dict(init=0)):
            assert _density(name, col0=2 ** 63 - 10, **kw) == SV_E_SHAPE and b"overflows" in L.lib().sv_last_error()


def test_entry_points_are_bound_and_exported():
    for name in ("sv_aggpost_sample", "sv_aggpost_scan", "sv_aggpost_dims", "sv_aggpost_finish"):
        assert name in L.EXPORTS and hasattr(L.lib(), name)
    assert L.lib().sv_version() == L.ABI_VERSION == 8
    assert S.AggregatePosterior is AG.AggregatePosterior and S.evaluate_aggregate is AG.evaluate_aggregate


# ================================================================================================ the Python layer
def test_partials_is_a_fixed_function_of_the_shapes():
    assert AG.partials(157, 50000) == 7 and AG.partials(626, 50000) == 2          # the bench shape: scan, dims
    assert AG.partials(2, 130) == 3 and AG.partials(1, 1) == 1 and AG.partials(1, 10 ** 6) == 64 and AG.partials(5000, 10 ** 6) == 1


def test_python_layer_refuses_cpu_tensors_and_bad_arguments():
    mu, ls = torch.zeros(4, 8), torch.zeros(4, 8)
    agg = S.AggregatePosterior(8)
    for fn in (lambda: agg.add(mu, ls), lambda: agg.sample(mu, ls), lambda: agg.log_density(mu)):
        with pytest.raises(L.ShotVaeHipError, match="MI355X|no CPU fallback"):
            fn()
    assert len(agg) == 0
    with pytest.raises(ValueError, match="dim must be >= 1"):
        S.AggregatePosterior(0)
    # the shape and range checks that need no tensor on the device (the others: tests/test_aggpost_gpu.py)
    for fn, word in ((lambda: agg.sample(None, None), "matrix"), (lambda: agg.log_density(None), "matrix"),
                     (lambda: agg.log_density([[0.0] * 8]), "matrix")):
        with pytest.raises(ValueError, match=word):
            fn()


def test_evaluate_aggregate_is_eval_mode_only_and_checks_its_arguments():
    x = torch.zeros(2, 3, 32, 32)
    vae = S.VariationalAutoEncoder("wideresnet-10-1", num_input_channels=3, img_size=(32, 32), data_parallel=False,
                                   continuous_latent_dim=128, disc_latent_dim=10, small_input=True, compute_dtype="fp32")
    smooth = S.SmoothVAE((SO.KINDS["svhn"]["in_ch"], 32, 32), {"cont": 32, "disc": [10]}, compute_dtype="fp32")
    for m in (vae, smooth):
        m.train()
        with pytest.raises(NotImplementedError, match="eval mode only"):
            S.evaluate_aggregate(m, [x])
        m.eval()
        with pytest.raises(L.ShotVaeHipError, match="MI355X"):
            S.evaluate_aggregate(m, [x])
        with pytest.raises(ValueError, match="empty"):
            S.evaluate_aggregate(m, [])
        for bad in (0, -1, 65537):
            with pytest.raises(ValueError, match="samples"):
                S.evaluate_aggregate(m, [x], samples=bad)
        with pytest.raises(ValueError, match="key"):
            S.evaluate_aggregate(m, [x], key=None)
        assert not m.training
    with pytest.raises(TypeError, match="VariationalAutoEncoder or a SmoothVAE"):
        S.evaluate_aggregate(torch.nn.Linear(2, 2), [x])
