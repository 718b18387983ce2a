"""Per-image scores without a GPU: the numpy restatement of sv_latent_sweep's normal stream and the float64 formulas of
sv_score_reduce (tests/_score_ref.py, written from the header comments of include/shotvae_hip.h; tests/test_score_gpu.py holds the
kernels to them) against known answers and the stream's properties,
the formulas on the reference's recorded terms (tests/golden/make_score_goldens.py), the argument checks of the three entry points,
and the eval-only API of score / log_likelihood / evaluate_scores."""
import math
import os

import numpy as np
import pytest
import torch

import shot_vae_amd as S
from shot_vae_amd import _lib as L
from oracle import closed_form as CF
from oracle import shotvae_oracle as O
from tests import _cases as T
from tests.golden import make_score_goldens as G
from tests._score_ref import lse, nll_rows, philox4x32_10, ref_scores, score_tag, sweep_lw, sweep_normals, sweep_z    # noqa: F401
from tests.test_infer_cpu import latent_normals, philox_tag

TOL = 2e-5                       # tests/test_oracle_golden.py: fp32 CPU against fp32 CPU
SV_E_ARG, SV_E_SHAPE = -1, -2    # include/shotvae_hip.h


# ------------------------------------------------------------------------------------------------ the stream's properties
def _philox_scalar(c, k):
    """Philox-4x32-10 on Python ints (Salmon et al., SC'11), independent of the array implementation"""
    c, k = list(c), list(k)
    for r in range(10):
        if r:
            k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
    return c


def _normal_scalar(key, row, s, d):
    r = _philox_scalar([row & 0xFFFFFFFF, row >> 32, (s << 16) | (d >> 2), score_tag()], [key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF])
    p = (d >> 1) & 1
    u1, u2 = ((r[2 * p] >> 8) + 1) * 2.0 ** -24, (r[2 * p + 1] >> 8) * 2.0 ** -24
    rad, ang = math.sqrt(-2.0 * math.log(u1)), 2.0 * math.pi * u2
    return rad * math.sin(ang) if d & 1 else rad * math.cos(ang)


# (key, row, s, d) -> n: worked once with the scalar restatement above (tag 0x53434F52), kept as constants so that neither restatement
# nor the tag can drift unnoticed
KNOWN_VALUES = {
    (0, 0, 0, 0): 0.5953653740381122,
    (1, 0, 0, 1): -1.2007101539279506,
    (0x5C0DE5EED1234, 3, 2, 127): -0.3807802707630348,
    (0x0123456789ABCDEF, 2 ** 32 + 5, 65535, 6): -0.1287689882307728,
    (-7, 11, 1, 2): 0.7957180300753218,
    (42, 7, 5, 3): 0.08204136203068942,
}


def test_known_answers():
    assert score_tag() == 0x53434F52
    for (key, row, s, d), want in KNOWN_VALUES.items():
        got = float(sweep_normals(key, row, 1, 1, d + 1, s0=s)[0, 0, d])
        assert abs(got - want) < 1e-12, ((key, row, s, d), got, want)
        assert abs(_normal_scalar(key & 0xFFFFFFFFFFFFFFFF, row, s, d) - want) < 1e-12


def test_counters_are_disjoint_from_dropout_and_latent_draw():
    """dropout: counters (q_lo, q_hi, unit, 0); sv_latent_draw: (row_lo, row_hi, d >> 2, SV_LATENT_PHILOX_TAG); the sweep's fourth word
    is a third value, so no counter is shared whatever the other three words are"""
    tag = score_tag()
    assert 0 < tag < 2 ** 32 and tag != philox_tag()
    c0 = np.arange(64, dtype=np.uint32)
    a = philox4x32_10(c0, 0, 3, 0, 1234, 5678)
    b = philox4x32_10(c0, 0, 3, philox_tag(), 1234, 5678)
    c = philox4x32_10(c0, 0, 3, tag, 1234, 5678)
    assert all(not np.any(x == z) and not np.any(y == z) for x, y, z in zip(a, b, c))
    # sample 0 of the sweep is not sv_latent_draw's stream
    assert not np.any(sweep_normals(77, 0, 4, 1, 128)[:, 0] == latent_normals(77, 0, 4, 128))


def test_values_do_not_depend_on_the_call_they_are_drawn_in():
    for ldc in (128, 5):
        whole = sweep_normals(77, 0, 12, 6, ldc)
        assert np.array_equal(whole, np.concatenate([sweep_normals(77, 0, 5, 6, ldc), sweep_normals(77, 5, 7, 6, ldc)]))
        assert np.array_equal(whole, np.concatenate([sweep_normals(77, 0, 12, 2, ldc), sweep_normals(77, 0, 12, 4, ldc, s0=2)], axis=1))
        assert not np.array_equal(whole, sweep_normals(78, 0, 12, 6, ldc))
        assert float(np.mean(whole[:, 0] == whole[:, 1])) == 0.0
    assert not np.array_equal(sweep_normals(77, 1, 1, 1, 8), sweep_normals(77, 1 + 2 ** 32, 1, 1, 8))
    # the two fields of the third counter word do not overlap at the limits S = 65536, ldc = 2^18
    assert ((65535 << 16) | ((2 ** 18 - 1) >> 2)) < 2 ** 32 and ((2 ** 18 - 1) >> 2) < (1 << 16)


def test_stream_is_standard_normal_and_finite():
    """2^20 draws: the standard error of the mean is 2^-10 = 9.8e-4 and of the variance sqrt(2) * 2^-10 = 1.4e-3, so the bounds are about
    five standard errors (the bounds of tests/test_infer_cpu.py)."""
    for dtype in (np.float64, np.float32):
        n = sweep_normals(0x1234567890ABCDEF, 0, 512, 16, 128, dtype)
        assert n.size == 2 ** 20 and np.isfinite(n).all()
        assert abs(float(n.mean(dtype=np.float64))) < 5e-3
        assert abs(float(n.var(dtype=np.float64)) - 1.0) < 1e-2
        assert float(np.abs(n).max()) <= math.sqrt(48 * math.log(2.0)) + 1e-5
    n = sweep_normals(5, 0, 512, 16, 128)
    assert abs(float(np.mean(n[:, 0] * n[:, 1]))) < 1e-2          # two samples of one image are uncorrelated


# ------------------------------------------------------------------------------------------------ formulas on the fixture
def test_fixture_is_small_and_complete():
    path = os.path.join(T.GOLDEN, G.TAG + ".npz")
    assert os.path.getsize(path) < 200 * 1024
    g = T.load(G.TAG)
    assert sorted(g.files) == sorted(["mu", "ls", "la", "z", "kl_c", "kl_d", "nll_mu_bce", "nll_mu_mse", "nll_s_bce", "nll_s_mse"])
    assert g["nll_s_bce"].shape == (G.B, G.S, G.K) and g["z"].shape == (G.B, G.S, G.LDC)
    assert all(np.isfinite(g[k]).all() for k in g.files)


def test_recorded_z_is_the_sweep_stream():
    g = T.load(G.TAG)
    z = sweep_z(G.KEY, G.ROW0, G.B, G.S, G.LDC, g["mu"], g["ls"])
    assert np.array_equal(z.astype(np.float32), g["z"])


def test_lw_is_the_log_density_ratio():
    """lw = log N(z; 0, I) - log N(z; mu, sigma^2), each written out as a density"""
    g = T.load(G.TAG)
    mu, ls = g["mu"].astype(np.float64)[:, None], g["ls"].astype(np.float64)[:, None]
    z = sweep_z(G.KEY, G.ROW0, G.B, G.S, G.LDC, g["mu"], g["ls"])
    log_p = (-0.5 * z * z - 0.5 * math.log(2 * math.pi)).sum(axis=2)
    log_q = (-0.5 * ((z - mu) / np.exp(ls)) ** 2 - ls - 0.5 * math.log(2 * math.pi)).sum(axis=2)
    lw = sweep_lw(G.KEY, G.ROW0, G.B, G.S, G.LDC, g["mu"], g["ls"])
    assert np.abs(lw - (log_p - log_q)).max() < 1e-9 * np.abs(lw).max()
    # without a key: z = mu
    lw0 = sweep_lw(None, 0, G.B, 1, G.LDC, g["mu"], g["ls"])
    assert np.allclose(lw0[:, 0], (-0.5 * mu * mu + ls).sum(axis=(1, 2)), rtol=1e-12)


def test_formulas_reproduce_the_recorded_kl_terms():
    g = T.load(G.TAG)
    out = ref_scores(g["nll_mu_bce"][:, None, :], None, g["la"], g["mu"], g["ls"])
    assert T.rel_err(out["kl_c"], g["kl_c"]) < TOL and T.rel_err(out["kl_d"], g["kl_d"]) < TOL
    q = np.exp(g["la"].astype(np.float64))
    assert np.allclose(out["recon"], (q * g["nll_mu_bce"]).sum(axis=1), rtol=1e-12)
    assert np.allclose(out["elbo"], -(out["recon"] + out["kl_c"] + out["kl_d"]), rtol=1e-12)
    for k in range(G.K):                                                          # labelled: the class's own term
        lab = ref_scores(g["nll_mu_bce"][:, None, k:k + 1], None, g["la"], g["mu"], g["ls"])
        assert np.allclose(lab["recon"], g["nll_mu_bce"][:, k], rtol=1e-12)


def test_log_px_on_the_recorded_terms():
    g = T.load(G.TAG)
    lw = sweep_lw(G.KEY, G.ROW0, G.B, G.S, G.LDC, g["mu"], g["ls"])
    for mode in ("bce", "mse"):
        nll = g["nll_s_" + mode].astype(np.float64)
        out = ref_scores(nll, lw, g["la"], g["mu"], g["ls"], add=1.5)
        inner = np.logaddexp.reduce(-nll - math.log(G.K), axis=2)                 # numpy's own stable pairwise form
        want = np.logaddexp.reduce(lw + inner, axis=1) - math.log(G.S) + 1.5
        assert np.allclose(out["log_px"], want, rtol=1e-12)
        lab = ref_scores(nll[:, :, 4:5], lw, g["la"], g["mu"], g["ls"])
        assert np.allclose(lab["log_px"], np.logaddexp.reduce(lw - nll[:, :, 4], axis=1) - math.log(G.S), rtol=1e-12)
        # Jensen: the bound with S samples is no smaller than the mean of the single-sample bounds
        single = (lw + inner).mean(axis=1) + 1.5
        assert (out["log_px"] >= single - 1e-9).all()


def test_inf_and_zero_probability_cases_by_hand():
    mu, ls = np.zeros((3, 2)), np.zeros((3, 2))                  # kl_c = 0
    la = np.log(np.array([[0.5, 0.5, 0.0], [1.0, 0.0, 0.0], [0.25, 0.25, 0.5]]), where=np.array([[1, 1, 0], [1, 0, 0], [1, 1, 1]], bool),
                out=np.full((3, 3), -np.inf))
    nll = np.array([[[2.0, 4.0, np.inf]], [[1.0, np.inf, np.inf]], [[np.inf, np.inf, np.inf]]])
    lw = np.zeros((3, 1))
    out = ref_scores(nll, lw, la, mu, ls)
    assert out["recon"][0] == 3.0 and out["recon"][1] == 1.0 and out["recon"][2] == np.inf       # q = 0 classes are skipped
    assert np.allclose(out["kl_d"], [math.log(3) - math.log(2), math.log(3), math.log(3) - 1.5 * math.log(2)], rtol=1e-12)
    assert np.isclose(out["log_px"][0], math.log((math.exp(-2) + math.exp(-4)) / 3))             # the +inf term has weight 0
    assert np.isclose(out["log_px"][1], -1.0 - math.log(3))
    assert out["log_px"][2] == -np.inf and out["elbo"][2] == -np.inf                             # not NaN
    assert not np.isnan(np.concatenate([v for v in out.values()])).any()
    # terms of magnitude 1e4 do not overflow
    big = ref_scores(np.full((1, 2, 3), 1.0e4), np.array([[-50.0, -60.0]]), la[2:], mu[:1], ls[:1])
    assert np.isclose(big["log_px"][0], -1.0e4 + math.log((math.exp(-50) + math.exp(-60)) / 2), rtol=1e-12)


def test_oracle_decoder_reproduces_the_recorded_terms():
    """the fixture's reconstruction terms from the CPU oracle's decoder (held to the reference by tests/test_infer_cpu.py) and the
    restated nll: every class at z = mu and at the recorded z"""
    g = T.load(G.TAG)
    st = CF.make_state(G.NAME, K=G.K)
    x = G.score_inputs().numpy()
    zs = np.concatenate([g["mu"][:, None], g["z"]], axis=1)                       # [B, 1 + S, ldc]
    lat = np.concatenate([np.repeat(zs[:, :, None], G.K, axis=2), np.broadcast_to(np.eye(G.K, dtype=np.float32), (G.B, 1 + G.S, G.K, G.K))],
                         axis=3).reshape(-1, G.LDC + G.K)
    with torch.no_grad():
        rec = O.decoder_forward(st, torch.from_numpy(lat)[:, :, None, None], training=False, update=False).numpy()
    xr = np.repeat(x, (1 + G.S) * G.K, axis=0)
    for mode, bce, sig in (("bce", True, 1.0), ("mse", False, G.X_SIGMA)):
        nll = nll_rows(rec, xr, bce, sig).reshape(G.B, 1 + G.S, G.K)
        assert T.rel_err(nll[:, 0], g["nll_mu_" + mode]) < TOL and T.rel_err(nll[:, 1:], g["nll_s_" + mode]) < TOL


# ------------------------------------------------------------------------------------------------ argument checks
PTR = 4096          # never dereferenced: a refused call launches nothing


def _sweep(**kw):
    a = dict(dtype=L.SV_BF16, mu=PTR, ls=PTR, key=PTR, row0=0, label=None, B=4, S=3, K=10, ldc=128, Lpad=144, j0=0, R=120, latent=PTR, lw=PTR)
    a.update(kw)
    return L.lib().sv_latent_sweep(a["dtype"], a["mu"], a["ls"], a["key"], a["row0"], a["label"], a["B"], a["S"], a["K"], a["ldc"], a["Lpad"],
                                   a["j0"], a["R"], a["latent"], a["lw"], None)


@pytest.mark.parametrize("kw,code,word", [
    (dict(mu=None), SV_E_ARG, b"mu or ls"), (dict(ls=None), SV_E_ARG, b"mu or ls"), (dict(latent=None), SV_E_ARG, b"output"),
    (dict(lw=None), SV_E_ARG, b"output"), (dict(dtype=2), SV_E_ARG, b"dtype"), (dict(B=0), SV_E_ARG, b"size"), (dict(S=0), SV_E_ARG, b"size"),
    (dict(K=-1), SV_E_ARG, b"size"), (dict(ldc=0), SV_E_ARG, b"size"), (dict(S=65537, R=1), SV_E_SHAPE, b"65536"),
    (dict(ldc=2 ** 18 + 1, Lpad=2 ** 19), SV_E_SHAPE, b"2^18"), (dict(Lpad=137), SV_E_SHAPE, b"Lpad"), (dict(row0=-1), SV_E_ARG, b"row0"),
    (dict(R=0), SV_E_SHAPE, b"rows"), (dict(j0=-1), SV_E_SHAPE, b"rows"), (dict(R=121), SV_E_SHAPE, b"rows"),
    (dict(j0=100, R=21), SV_E_SHAPE, b"rows"), (dict(label=PTR, R=13), SV_E_SHAPE, b"rows")])
def test_latent_sweep_refuses_bad_arguments_before_any_launch(kw, code, word):
    assert _sweep(**kw) == code and word in L.lib().sv_last_error()


def _recon(**kw):
    a = dict(dtype=L.SV_BF16, rec=PTR, image=PTR, B=4, j0=0, R=120, rpi=30, C=3, H=32, W=32, ld=16, bce=1, x_sigma=1.0, nll=PTR)
    a.update(kw)
    return L.lib().sv_recon_rows(a["dtype"], a["rec"], a["image"], a["B"], a["j0"], a["R"], a["rpi"], a["C"], a["H"], a["W"], a["ld"], a["bce"],
                                 a["x_sigma"], a["nll"], None)


@pytest.mark.parametrize("kw,code,word", [
    (dict(rec=None), SV_E_ARG, b"pointer"), (dict(image=None), SV_E_ARG, b"pointer"), (dict(nll=None), SV_E_ARG, b"pointer"),
    (dict(dtype=-1), SV_E_ARG, b"dtype"), (dict(B=0), SV_E_ARG, b"size"), (dict(R=0), SV_E_ARG, b"size"), (dict(C=0), SV_E_ARG, b"size"),
    (dict(H=-3), SV_E_ARG, b"size"), (dict(W=0), SV_E_ARG, b"size"), (dict(rpi=0), SV_E_ARG, b"size"), (dict(ld=2), SV_E_SHAPE, b"ld="),
    (dict(bce=2), SV_E_ARG, b"bce"), (dict(bce=0, x_sigma=0.0), SV_E_ARG, b"x_sigma"), (dict(bce=0, x_sigma=float("nan")), SV_E_ARG, b"x_sigma"),
    (dict(bce=0, x_sigma=float("inf")), SV_E_ARG, b"x_sigma"), (dict(R=121), SV_E_SHAPE, b"past image"), (dict(j0=-1), SV_E_SHAPE, b"past image"),
    (dict(j0=119, R=2), SV_E_SHAPE, b"past image")])
def test_recon_rows_refuses_bad_arguments_before_any_launch(kw, code, word):
    assert _recon(**kw) == code and word in L.lib().sv_last_error()


def _reduce(**kw):
    a = dict(nll=PTR, lw=PTR, la=PTR, mu=PTR, ls=PTR, B=4, S=3, Kd=10, K=10, ldc=128, add=0.0, recon=PTR, kl_c=PTR, kl_d=PTR, elbo=PTR,
             log_px=PTR)
    a.update(kw)
    return L.lib().sv_score_reduce(a["nll"], a["lw"], a["la"], a["mu"], a["ls"], a["B"], a["S"], a["Kd"], a["K"], a["ldc"], a["add"],
                                   a["recon"], a["kl_c"], a["kl_d"], a["elbo"], a["log_px"], None)


@pytest.mark.parametrize("kw,code,word", [
    (dict(nll=None), SV_E_ARG, b"input"), (dict(la=None), SV_E_ARG, b"input"), (dict(mu=None), SV_E_ARG, b"input"),
    (dict(ls=None), SV_E_ARG, b"input"), (dict(recon=None, kl_c=None, kl_d=None, elbo=None, log_px=None), SV_E_ARG, b"no output"),
    (dict(lw=None), SV_E_ARG, b"needs lw"), (dict(B=0), SV_E_ARG, b"size"), (dict(S=0), SV_E_ARG, b"size"), (dict(Kd=0), SV_E_ARG, b"size"),
    (dict(K=0), SV_E_ARG, b"size"), (dict(ldc=-2), SV_E_ARG, b"size"), (dict(Kd=5), SV_E_SHAPE, b"Kd=5"),
    (dict(add=float("nan")), SV_E_ARG, b"finite"), (dict(add=float("-inf")), SV_E_ARG, b"finite")])
def test_score_reduce_refuses_bad_arguments_before_any_launch(kw, code, word):
    assert _reduce(**kw) == code and word in L.lib().sv_last_error()


# ------------------------------------------------------------------------------------------------ API
def _model():
    return S.VariationalAutoEncoder(G.NAME, num_input_channels=3, img_size=(32, 32), data_parallel=False, continuous_latent_dim=G.LDC,
                                    disc_latent_dim=G.K, small_input=True, compute_dtype="fp32")


def _calls(m, x=None, key=None, **kw):
    x = torch.zeros(2, 3, 32, 32) if x is None else x
    key = torch.zeros(1, dtype=torch.int64) if key is None else key
    crit = S.VAECriterion(discrete_dim=G.K)
    return {"score": lambda: m.score(x, crit, **kw), "score sampled": lambda: m.score(x, crit, samples=2, key=key, **kw),
            "log_likelihood": lambda: m.log_likelihood(x, crit, 2, key, **kw),
            "score_terms": lambda: m.score_terms(x, crit, ("elbo", "log_px"), samples=2, key=key, **kw)}


def test_exports():
    assert S.Scores._fields == ("recon", "kl_c", "kl_d", "elbo") and callable(S.evaluate_scores)
    for name in ("sv_latent_sweep", "sv_recon_rows", "sv_score_reduce"):
        assert name in L.EXPORTS and hasattr(L.lib(), name)


def test_score_calls_are_eval_mode_only():
    m = _model().train()
    for name, fn in _calls(m).items():
        with pytest.raises(NotImplementedError, match=r"model\.eval\(\)"):
            fn()


def test_evaluate_scores_is_eval_mode_only_and_needs_data():
    m, crit = _model().train(), S.VAECriterion(discrete_dim=G.K)
    with pytest.raises(NotImplementedError, match=r"model\.eval\(\)"):
        S.evaluate_scores(m, crit, [torch.zeros(2, 3, 32, 32)])
    assert m.training, "evaluate_scores switched the model's mode"
    with pytest.raises(ValueError, match="empty"):
        S.evaluate_scores(m.eval(), crit, [])


def test_default_chunk_stays_under_the_documented_scratch():
    """a decoded row of wideresnet-28-2 holds 110880 bytes of eval scratch in bf16 and 221760 in fp32 -- the latent, the six
    layers' outputs and the materialised inputs of layers 1 to 3 -- so the default chunk stays under 1 GB / 2 GB"""
    for dt, want in (("bf16", 110880), ("fp32", 221760)):
        eng = S.VariationalAutoEncoder("wideresnet-28-2", num_input_channels=3, img_size=(32, 32), continuous_latent_dim=128,
                                       disc_latent_dim=10, small_input=True, compute_dtype=dt)._engine
        es = 2 if dt == "bf16" else 4
        by_hand = es * (144 + 1024 + 4 * 512 + 16 * 256 + 64 * 128 + 256 * 64 + 1024 * 16 + 1024 + 4 * 512 + 16 * 256)
        assert eng.decoder_row_bytes() == want == by_hand
        assert eng.SCORE_CHUNK_ROWS == 8192 and eng.SCORE_CHUNK_ROWS * want < (1e9 if dt == "bf16" else 2e9)


def test_score_calls_refuse_cpu_tensors():
    m = _model().eval()
    for name, fn in _calls(m).items():
        with pytest.raises(L.ShotVaeHipError, match=r"\.%s:" % name.split()[0]):
            fn()
    with pytest.raises(L.ShotVaeHipError, match="evaluate_scores"):
        S.evaluate_scores(m, S.VAECriterion(discrete_dim=G.K), [(torch.zeros(2, 3, 32, 32), torch.zeros(2))])
    assert not m.training


def test_score_calls_check_their_arguments():
    m, crit, x = _model().eval(), S.VAECriterion(discrete_dim=G.K), torch.zeros(2, 3, 32, 32)
    key = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ValueError, match="needs a key"):
        m.score(x, crit, samples=2)
    with pytest.raises(ValueError, match="key is required"):
        m.log_likelihood(x, crit, 2, None)
    for bad in (torch.zeros(1, dtype=torch.int32), torch.zeros(1), torch.zeros(2, dtype=torch.int64), 2.5, True, "7"):
        with pytest.raises(ValueError, match="1-element int64"):
            m.score(x, crit, samples=2, key=bad)
        with pytest.raises(ValueError, match="1-element int64"):
            m.log_likelihood(x, crit, 2, bad)
    for s in (0, 65537):
        with pytest.raises(ValueError, match="samples"):
            m.log_likelihood(x, crit, s, key)
    with pytest.raises(ValueError, match="label"):
        m.score(x, crit, label=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="label"):
        m.score(x, crit, label=torch.zeros(2))
    with pytest.raises(ValueError, match="images"):
        m.score(torch.zeros(2, 1, 32, 32), crit)
    with pytest.raises(ValueError, match="classes"):
        m.score(x, S.VAECriterion(discrete_dim=7))
    with pytest.raises(ValueError, match="row0"):
        m.score(x, crit, row0=-1)
    with pytest.raises(ValueError, match="key"):
        S.evaluate_scores(m, crit, [x], samples=2)
