"""Linear probes without a GPU: the float64 restatement of tests/_probe_ref.py pinned to torch.autograd, to finite differences and to
scikit-learn, its identities, the label budget, the stopping rule, the argument refusals of the three sv_probe_* entry points (they
validate before any HIP call) and the host logic of shot_vae_amd.probe."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import shot_vae_amd as S
from shot_vae_amd import _lib as L
from shot_vae_amd import probe as PB
from tests import _probe_ref as R

SV_E_ARG, SV_E_SHAPE = -1, -2


def point(K, D, seed, size=0.5):
    return np.random.default_rng(seed).normal(0.0, size, (K, D + 1))


# ================================================================================================ against references
def test_the_restated_gradient_is_autograds():
    for N, K, D, lam in ((40, 3, 5, 0.1), (70, 17, 9, 1e-3)):
        x, y = R.overlapping(N, K, D, 9101)
        y[3] = -1
        t = point(K, D, 9102)
        tt = torch.tensor(t, dtype=torch.float64, requires_grad=True)
        ok = torch.from_numpy(R.used_rows(x, y, K))
        logits = torch.from_numpy(x)[ok] @ tt[:, 1:].T + tt[:, 0]
        loss = torch.nn.functional.cross_entropy(logits, torch.from_numpy(y)[ok]) + 0.5 * lam * (tt[:, 1:] ** 2).sum()
        loss.backward()
        err_f, err_g = abs(R.objective(x, y, t, lam) - float(loss.detach())),float(np.abs(R.gradient(x, y, t, lam) - tt.grad.numpy()).max())
        print("FIG restatement against autograd %s: objective %.1e gradient %.1e" % ((N, K, D), err_f, err_g))
        assert err_f <= 1e-12 and err_g <= 1e-12


def test_the_restated_gradient_matches_central_differences_of_its_own_objective():
    N, K, D, lam = 50, 4, 3, 0.05
    x, y = R.overlapping(N, K, D, 9103)
    t = point(K, D, 9104)
    g = R.gradient(x, y, t, lam)
    h, worst = 1e-5, 0.0
    for k in range(K):
        for e in range(D + 1):
            up, dn = t.copy(), t.copy()
            up[k, e] += h
            dn[k, e] -= h
            worst = max(worst, abs((R.objective(x, y, up, lam) - R.objective(x, y, dn, lam)) / (2 * h) - g[k, e]))
    print("FIG central differences: %.1e" % worst)
    assert worst <= 1e-8          # h^2 |F'''| / 6 with |F'''| of order 1, plus eps |F| / h = 2e-11


def test_loss_and_probabilities_are_scikit_learns_at_its_own_coefficients():
    lm = pytest.importorskip("sklearn.linear_model")
    metrics = pytest.importorskip("sklearn.metrics")
    x, y = R.overlapping(120, 4, 6, 9105)
    sk = lm.LogisticRegression(C=1.0, max_iter=200).fit(x, y)
    lse, loss, pred, proba = R.rows(x, sk.coef_, sk.intercept_, y)
    assert np.abs(proba - sk.predict_proba(x)).max() <= 1e-12 and np.array_equal(pred, sk.predict(x))
    assert abs(loss.mean() - metrics.log_loss(y, sk.predict_proba(x))) <= 1e-12


@pytest.mark.parametrize("N,K,D,Cc,iters", [(300, 3, 5, 1.0, 400), (512, 10, 16, 1.0, 1500), (193, 17, 33, 0.1, 800)])
def test_the_restated_fit_reaches_scikit_learns_optimum(N, K, D, Cc, iters):
    """on standardised rows; the intercepts are centred on both sides: their common shift is free"""
    lm = pytest.importorskip("sklearn.linear_model")
    x, y = R.overlapping(N, K, D, 9107)
    rows, mean, scale, lam, lip, beta = R.constants(x, y, K, Cc)
    theta, look, seen = R.nesterov(rows, y, K, lam, lip, beta, iters)
    sk = lm.LogisticRegression(C=Cc, tol=1e-12, max_iter=100000).fit(rows, y)
    b_sk = sk.intercept_ - sk.intercept_.mean()
    err = max(float(np.abs(look[:, 1:] - sk.coef_).max()), float(np.abs(look[:, 0] - look[:, 0].mean() - b_sk).max()))
    print("FIG fit against scikit-learn %s C=%g after %d iterations: %.1e, max |g| %.1e, kappa %.0f"
          % ((N, K, D), Cc, iters, err, seen[-1], lip / lam))
    assert err <= 1e-5
    assert float(np.abs(R.gradient(rows, y, look, lam)).max()) <= 1e-6


# ================================================================================================ identities
def test_the_class_gradients_sum_to_zero_and_a_common_shift_changes_no_probability():
    x, y = R.overlapping(80, 5, 7, 9109)
    t = point(5, 7, 9110)
    g = R.gradient(x, y, t, 0.0)
    assert np.abs(g.sum(axis=0)).max() <= 1e-15
    shift = np.random.default_rng(9111).normal(size=8)
    p0 = R.rows(x, t[:, 1:], t[:, 0])[3]
    p1 = R.rows(x, (t + shift[None, :])[:, 1:], (t + shift[None, :])[:, 0])[3]
    assert np.abs(p0 - p1).max() <= 1e-13 and np.abs(p0.sum(axis=1) - 1.0).max() <= 1e-14


def test_merging_partial_states_is_exact_in_the_restatement():
    """integer rows and dyadic residuals: every sum is exact, so any P and any cut give the same merged state"""
    rng = np.random.default_rng(9113)
    x = np.floor(rng.uniform(-4, 5, (300, 3)))
    r = rng.integers(-4, 5, (300, 4)) / 4.0
    y = rng.integers(0, 4, 300)
    lse, loss = rng.integers(-8, 8, 300) / 2.0, rng.integers(0, 16, 300) / 4.0
    lse[[5, 70]] = np.nan
    y[9] = -1
    one = R.merge(R.accum(x, r, y, lse, loss, 1)[0])
    for P in (2, 3, 5):
        sums, counts = R.accum(x, r, y, lse, loss, P)
        assert np.array_equal(R.merge(sums), one) and counts.sum(axis=0).tolist() == [297, 3]
        a, ca = R.accum(x[:64 * P], r[:64 * P], y[:64 * P], lse[:64 * P], loss[:64 * P], P)
        b, cb = R.accum(x[64 * P:], r[64 * P:], y[64 * P:], lse[64 * P:], loss[64 * P:], P, a, ca)
        assert np.array_equal(b, sums) and np.array_equal(cb, counts)
    ok = np.isfinite(lse) & (y >= 0)
    body = one[:-1].reshape(4, 4)
    assert np.array_equal(body[:, 0], r[ok].sum(axis=0)) and np.array_equal(body[:, 1:], r[ok].T @ x[ok]) and one[-1] == loss[ok].sum()


def test_unlabelled_rows_change_nothing_but_the_skip_count():
    x, y = R.overlapping(100, 3, 4, 9115)
    t = point(3, 4, 9116)
    more_x = np.concatenate([x[:30], np.full((7, 4), 5.0), x[30:]])
    more_y = np.concatenate([y[:30], np.array([-1, 3, -1, 99, -5, 3, -1]), y[30:]])
    assert R.objective(more_x, more_y, t, 0.1) == R.objective(x, y, t, 0.1)
    assert np.array_equal(R.gradient(more_x, more_y, t, 0.1), R.gradient(x, y, t, 0.1))
    states = []
    for rows_, lab in ((x, y), (more_x, more_y)):
        lse, loss, _, _ = R.rows(rows_, t[:, 1:], t[:, 0], lab)
        r = R.residuals(rows_, t[:, 1:], t[:, 0], lab)
        states.append(R.accum(rows_, r, lab, lse, np.nan_to_num(loss), 1))
    assert np.array_equal(states[0][0], states[1][0]) and states[0][1].tolist() == [[100, 0]] and states[1][1].tolist() == [[100, 7]]
    out = R.update(states[1][0], states[1][1], 3, 4, 0.1, 0.5, 0.3, t, t)
    assert np.abs(out[0] - R.gradient(x, y, t, 0.1)).max() <= 1e-15 and abs(out[5][0] - R.objective(x, y, t, 0.1)) <= 1e-14
    assert out[5][2] == 100 and out[5][3] == 7 and out[5][1] == np.abs(out[0]).max()
    # no used row: the model stays, the statistics are NaN
    none = R.update(np.zeros((2, R.state_stride(3, 4))), np.array([[0, 5], [0, 2]]), 3, 4, 0.1, 0.5, 0.3, t, t + 1)
    assert np.array_equal(none[1], t) and np.array_equal(none[2], t + 1) and np.isnan(none[5][:2]).all() and none[5][2:4].tolist() == [0, 7]


# ================================================================================================ the label budget
def test_the_budget_keeps_m_rows_per_class_is_seeded_and_nested():
    rng = np.random.default_rng(9117)
    y = torch.from_numpy(rng.integers(0, 5, 400))
    y[::17] = -1
    y[3] = 7
    previous = None
    for m in (1, 3, 10, 1000):
        kept = PB.select_labels(y, m, 5, seed=4)
        on = kept >= 0
        assert torch.equal(kept[on], y[on]) and bool((kept[~on] == -1).all())
        want = [min(m, int((y == c).sum())) for c in range(5)]
        assert [int((kept == c).sum()) for c in range(5)] == want
        assert torch.equal(kept, PB.select_labels(y, m, 5, seed=4))
        if previous is not None:
            assert bool(on[previous].all())
        previous = on
    assert not torch.equal(PB.select_labels(y, 3, 5, seed=4), PB.select_labels(y, 3, 5, seed=5))
    valid = (y >= 0) & (y < 5)
    assert torch.equal(PB.select_labels(y, 1000, 5, seed=4)[valid], y[valid])
    for bad in (lambda: PB.select_labels(y.double(), 3, 5), lambda: PB.select_labels(y, 0, 5), lambda: PB.select_labels(y[None], 3, 5)):
        with pytest.raises(ValueError):
            bad()


# ================================================================================================ the stopping rule
def scripted(values, **kw):
    reads, it = [], iter(values)
    def read(handle):
        reads.append(handle)
        return handle
    n, conv = PB._probe_loop(lambda: next(it), read, **kw)
    return n, conv, reads


def test_fit_stops_by_the_gradient_rule_on_a_scripted_sequence():
    seq = [1.0, 0.1, 1e-5, 0.5, 1e-6, 1e-7]
    assert scripted(seq, max_iter=6, tol=1e-4, check_every=1) == (3, True, [1.0, 0.1, 1e-5])
    assert scripted(seq, max_iter=6, tol=1e-4, check_every=2) == (6, True, [0.1, 0.5, 1e-7])       # iteration 3 is not a checked one
    assert scripted(seq, max_iter=5, tol=1e-4, check_every=4) == (5, True, [0.5, 1e-6])            # the last iteration is always checked
    assert scripted(seq, max_iter=4, tol=1e-4, check_every=4) == (4, False, [0.5])
    assert scripted(seq, max_iter=6, tol=1e-4, check_every=3) == (3, True, [1e-5])
    assert scripted(seq, max_iter=6, tol=None, check_every=1) == (6, False, [])                     # never with tol=None
    assert scripted([float("nan")] * 3, max_iter=3, tol=1e-4, check_every=1)[:2] == (3, False)      # a NaN gradient never converges
    assert scripted([1e-4], max_iter=1, tol=1e-4, check_every=1)[:2] == (1, False)                  # strictly below tol


def test_step_constants_are_boehnings_bound_and_the_constant_momentum():
    lip, beta = PB.step_constants(3.0, 0.5)
    assert lip == 2.0 and beta == (1 - 0.5) / (1 + 0.5)
    x, y = R.overlapping(60, 3, 4, 9119)
    rows, mean, scale, lam, lip, beta = R.constants(x, y, 3, 2.0)
    assert lam == 1.0 / 120 and np.abs(rows.mean(axis=0)).max() <= 1e-6 and np.abs(rows.std(axis=0) - 1).max() <= 1e-6
    # Boehning: the Hessian of the softmax loss is below 1/2 (I - 1 1'/K) (x) Gram, whose largest eigenvalue is at most eigmax / 2
    t = point(3, 4, 9120)
    p = R.rows(rows, t[:, 1:], t[:, 0])[3]
    aug = np.concatenate([np.ones((60, 1)), rows], axis=1)
    H = sum(np.kron(np.diag(pi) - np.outer(pi, pi), np.outer(a, a)) for pi, a in zip(p, aug)) / 60
    assert np.linalg.eigvalsh(H)[-1] <= lip - lam + 1e-12 and 0 < beta < 1


# ================================================================================================ the entry points' refusals
P4 = C.c_void_p(4096)               # never dereferenced: nothing is launched


def _rows(**kw):
    a = dict(x=P4, N=5, w=P4, b=P4, K=3, D=4, label=P4, lse=P4, loss=None, pred=None, proba=None)
    a.update(kw)
    return L.lib().sv_probe_rows(a["x"], a["N"], a["w"], a["b"], a["K"], a["D"], a["label"], a["lse"], a["loss"], a["pred"], a["proba"], None)


def _accum(**kw):
    a = dict(x=P4, label=P4, lse=P4, loss=P4, N=5, w=P4, b=P4, K=3, D=4, sums=P4, counts=P4, P=2, init=1, resid=None)
    a.update(kw)
    return L.lib().sv_probe_accum(a["x"], a["label"], a["lse"], a["loss"], a["N"], a["w"], a["b"], a["K"], a["D"], a["sums"], a["counts"],
                                  a["P"], a["init"], a["resid"], None)


def _update(**kw):
    a = dict(sums=P4, counts=P4, P=2, K=3, D=4, lam=0.1, inv_L=0.5, beta=0.3, theta=P4, look=P4, w=P4, b=P4, stats=P4)
    a.update(kw)
    return L.lib().sv_probe_update(a["sums"], a["counts"], a["P"], a["K"], a["D"], a["lam"], a["inv_L"], a["beta"], a["theta"], a["look"],
                                   a["w"], a["b"], a["stats"], None)


REFUSALS = [
    (_rows, "sv_probe_rows", [(dict(x=None), SV_E_ARG, b"NULL"), (dict(w=None), SV_E_ARG, b"NULL"), (dict(b=None), SV_E_ARG, b"NULL"),
                              (dict(lse=None), SV_E_ARG, b"lse"), (dict(label=None, loss=P4), SV_E_ARG, b"loss without label"),
                              (dict(N=0), SV_E_ARG, b"size"), (dict(D=0), SV_E_ARG, b"size"), (dict(K=1), SV_E_ARG, b"K=1"),
                              (dict(K=0), SV_E_ARG, b"K=0")]),
    (_accum, "sv_probe_accum", [(dict(x=None), SV_E_ARG, b"NULL"), (dict(label=None), SV_E_ARG, b"NULL"), (dict(lse=None), SV_E_ARG, b"NULL"),
                                (dict(loss=None), SV_E_ARG, b"NULL"), (dict(w=None), SV_E_ARG, b"NULL"), (dict(b=None), SV_E_ARG, b"NULL"),
                                (dict(sums=None), SV_E_ARG, b"NULL"), (dict(counts=None), SV_E_ARG, b"NULL"), (dict(N=0), SV_E_ARG, b"size"),
                                (dict(D=-1), SV_E_ARG, b"size"), (dict(K=1), SV_E_ARG, b"K=1"), (dict(P=0), SV_E_ARG, b"P=0"),
                                (dict(P=65), SV_E_ARG, b"P=65"), (dict(D=(1 << 20) + 1), SV_E_SHAPE, b"2^20"),
                                (dict(K=1 << 20, D=1 << 12), SV_E_SHAPE, b"31 bits")]),
    (_update, "sv_probe_update", [(dict(sums=None), SV_E_ARG, b"NULL"), (dict(counts=None), SV_E_ARG, b"NULL"), (dict(theta=None), SV_E_ARG, b"NULL"),
                                  (dict(look=None), SV_E_ARG, b"NULL"), (dict(w=None), SV_E_ARG, b"NULL"), (dict(b=None), SV_E_ARG, b"NULL"),
                                  (dict(stats=None), SV_E_ARG, b"stats"), (dict(D=0), SV_E_ARG, b"size"), (dict(K=1), SV_E_ARG, b"K=1"),
                                  (dict(P=0), SV_E_ARG, b"P=0"), (dict(P=65), SV_E_ARG, b"P=65"), (dict(lam=0.0), SV_E_ARG, b"lambda"),
                                  (dict(lam=float("nan")), SV_E_ARG, b"lambda"), (dict(lam=float("inf")), SV_E_ARG, b"lambda"),
                                  (dict(inv_L=-1.0), SV_E_ARG, b"inv_L"), (dict(inv_L=float("inf")), SV_E_ARG, b"inv_L"),
                                  (dict(beta=1.0), SV_E_ARG, b"beta"), (dict(beta=-0.1), SV_E_ARG, b"beta"), (dict(beta=float("nan")), SV_E_ARG, b"beta"),
                                  (dict(D=(1 << 20) + 1), SV_E_SHAPE, b"2^20"), (dict(K=1 << 20, D=1 << 12), SV_E_SHAPE, b"31 bits")]),
]


@pytest.mark.parametrize("fn,name,cases", REFUSALS, ids=[r[1] for r in REFUSALS])
def test_entry_points_refuse_bad_arguments_before_any_launch(fn, name, cases):
    for kw, code, word in cases:
        assert fn(**kw) == code, (name, kw)
        err = L.lib().sv_last_error()
        assert word in err and name.encode() in err, (kw, err)


def test_entry_points_are_bound_and_exported():
    for name in ("sv_probe_rows", "sv_probe_accum", "sv_probe_update"):
        assert name in L.EXPORTS and hasattr(L.lib(), name)
    assert L.lib().sv_version() == L.ABI_VERSION == 8
    for name in ("LinearProbe", "evaluate_probe", "select_labels"):
        assert getattr(S, name) is getattr(PB, name)


# ================================================================================================ host logic
def test_partials_are_a_function_of_the_shapes():
    for k, d, n in ((10, 128, 50000), (100, 640, 50000), (3, 5, 200), (1000, 512, 10 ** 6)):
        p = PB._partials(k, d, n)
        blocks = (1 if k <= 16 else -(-k // 64)) * -(-d // 32)
        assert 1 <= p <= 64 and p <= -(-n // 64) and (p == 1 or p * blocks <= 512) and p == PB._partials(k, d, n)
    assert PB._partials(10, 128, 50000) == 64 and PB._partials(3, 5, 100) == 2


def test_python_layer_refuses_bad_arguments():
    for k, d in ((1, 4), (0, 4), (2, 0), (2, (1 << 20) + 1), (1 << 14, 1 << 17)):
        with pytest.raises(ValueError):
            S.LinearProbe(k, d)
    for c in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="C must be"):
            S.LinearProbe(2, 4, C=c)
    lp = S.LinearProbe(3, 4)
    x, y = torch.zeros(6, 4), torch.zeros(6, dtype=torch.int64)
    with pytest.raises(ValueError, match=">= 1"):
        lp.fit(x, y, max_iter=0)
    with pytest.raises(ValueError, match=">= 1"):
        lp.fit(x, y, check_every=0)
    with pytest.raises(ValueError, match="tol"):
        lp.fit(x, y, tol=-1.0)
    with pytest.raises(ValueError, match="no parameters"):
        lp.state_dict()
    with pytest.raises(ValueError, match="no parameters"):
        lp.predict(x)
    with pytest.raises(ValueError, match="lambda"):
        lp.start("cuda", 0.0, 1.0, 0.5)
    with pytest.raises(L.ShotVaeHipError, match="MI355X"):
        lp.start("cpu", 0.1, 1.0, 0.5)
    with pytest.raises(TypeError):
        S.evaluate_probe(object(), [], [])


def test_python_layer_checks_shapes_before_it_asks_for_the_device():
    x, y = torch.zeros(6, 4), torch.zeros(6, dtype=torch.int64)
    lp = S.LinearProbe(3, 4)
    with pytest.raises(ValueError, match="columns"):
        S.LinearProbe(3, 5).fit(x, y)
    with pytest.raises(ValueError, match="matrix"):
        lp.fit(x.view(-1), y)
    with pytest.raises(ValueError, match="matrix"):
        lp.fit([[0.0] * 4] * 6, y)
    # ... and then the no-CPU rule
    with pytest.raises(L.ShotVaeHipError, match="MI355X"):
        lp.fit(x, y)
    sd = dict(k=3, dim=4, w=torch.zeros(3, 4), b=torch.zeros(3), mean=torch.zeros(4), scale=torch.ones(4), converged=True, n_iter=9)
    lp.load_state_dict(sd)
    assert lp.converged_ is True and lp.n_iter_ == 9
    for call in (lambda: lp.predict(x), lambda: lp.predict_proba(x), lambda: lp.decision_function(x), lambda: lp.score(x, y),
                 lambda: lp.log_loss(x, y), lambda: lp.step(x, y)):
        with pytest.raises(L.ShotVaeHipError, match="MI355X"):
            call()
    with pytest.raises(ValueError, match="columns"):
        lp.predict(torch.zeros(6, 5))
    with pytest.raises(ValueError, match="3 x 4"):
        S.LinearProbe(2, 4).load_state_dict(sd)
    with pytest.raises(ValueError, match="mean"):
        S.LinearProbe(3, 4).load_state_dict(dict(sd, mean=torch.zeros(3)))


def test_state_dict_round_trip_and_raw_coordinates_on_the_host():
    rng = np.random.default_rng(9121)
    lp = S.LinearProbe(3, 4, C=2.0)
    sd = dict(k=3, dim=4, C=0.5, standardize=True, w=torch.from_numpy(rng.normal(size=(3, 4))).float(), b=torch.from_numpy(rng.normal(size=3)).float(),
              mean=torch.from_numpy(rng.normal(size=4)), scale=torch.from_numpy(rng.uniform(0.5, 2, 4)))
    lp.load_state_dict(sd)
    out = lp.state_dict()
    other = S.LinearProbe(3, 4).load_state_dict(out)
    for name in ("w", "b", "mean", "scale"):
        assert torch.equal(getattr(other, name), getattr(lp, name)) and getattr(other, name) is not out[name]
    assert other.C == 0.5 and torch.equal(other.theta[:, 0], lp.b.double()) and torch.equal(other.look[:, 1:], lp.w.double())
    # (coef_ / intercept_ ask for the device first: the translation itself is restated here)
    x = rng.normal(size=(5, 4))
    w, b, mean, scale = (getattr(lp, n).double().numpy() for n in ("w", "b", "mean", "scale"))
    coef, intercept = w / scale, b - (w * (mean / scale)).sum(axis=1)
    assert np.abs((x @ coef.T + intercept) - (((x - mean) / scale) @ w.T + b)).max() <= 1e-13
