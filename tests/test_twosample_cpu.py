"""Kernel two-sample statistics without a GPU: the float64 restatement of tests/_twosample_ref.py pinned to scikit-learn's kernels and
to hand-written sums, its identities, the exact fmaf emulation, the analytic prior expectations against a Monte-Carlo mean, the inputs
of the GPU tests checked against their own conditions, the argument refusals of sv_ksum_scan / sv_ksum_finish (they validate before any
HIP call) and the host logic of shot_vae_amd.twosample."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

import shot_vae_amd as S
from shot_vae_amd import _lib as L
from shot_vae_amd import twosample as TS
from tests import _twosample_ref as R

SV_E_ARG, SV_E_SHAPE = -1, -2


def rnd(n, D, seed, scale=1.0):
    return (scale * np.random.RandomState(seed).randn(n, D)).astype(np.float32).astype(np.float64)


# ================================================================================================ against scikit-learn and by hand
def test_the_dense_restatement_is_scikit_learns_kernels():
    P = pytest.importorskip("sklearn.metrics.pairwise")
    x, y = rnd(23, 7, 1), rnd(31, 7, 2)
    for a in (0.05, 0.7):
        got = R.kernel_matrix(R.RBF, R.params(R.RBF, [a]), 0, x, y)
        assert np.abs(got - P.rbf_kernel(x, y, gamma=a)).max() <= 1e-12
    for degree, gamma, coef0 in ((1, 0.3, 0.0), (3, 1.0 / 7, 1.0), (2, 0.5, 2.0)):
        got = R.kernel_matrix(R.POLY, R.params(R.POLY, gamma, coef0), degree, x, y)
        want = P.polynomial_kernel(x, y, degree=degree, gamma=gamma, coef0=coef0)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    ladder = R.params(R.RBF, [0.1, 0.2, 0.4])
    want = sum(P.rbf_kernel(x, y, gamma=a) for a in (0.1, 0.2, 0.4)) / 3.0
    assert np.abs(R.kernel_matrix(R.RBF, ladder, 0, x, y) - want).max() <= 1e-12
    imq = R.kernel_matrix(R.IMQ, R.params(R.IMQ, [0.5]), 0, x, y)
    assert np.abs(imq - 1.0 / (1.0 + 0.5 * P.euclidean_distances(x, y, squared=True))).max() <= 1e-12


def test_mmd2_on_five_rows_by_hand():
    x, y = rnd(5, 3, 3), rnd(5, 3, 4) + 0.5
    a = 0.4
    k = lambda u, v: np.exp(-a * np.sum((u - v) ** 2))          # noqa: E731
    n = m = 5
    sxx_u = sum(k(x[i], x[j]) for i in range(n) for j in range(n) if i != j)
    syy_u = sum(k(y[i], y[j]) for i in range(m) for j in range(m) if i != j)
    sxy = sum(k(x[i], y[j]) for i in range(n) for j in range(m))
    kp = R.params(R.RBF, [a])
    assert abs(R.mmd2(R.RBF, kp, 0, x, y, True) - (sxx_u / 20 + syy_u / 20 - 2 * sxy / 25)) <= 1e-14
    assert abs(R.mmd2(R.RBF, kp, 0, x, y, False) - ((sxx_u + 5) / 25 + (syy_u + 5) / 25 - 2 * sxy / 25)) <= 1e-14
    at = rnd(4, 3, 5)
    want = [np.mean([k(t, r) for r in x]) - np.mean([k(t, r) for r in y]) for t in at]
    assert np.abs(R.witness(R.RBF, kp, 0, x, y, at) - want).max() <= 1e-14


def test_the_kid_restatement_follows_the_formulas():
    real, fake = rnd(40, 6, 6), rnd(30, 6, 7) * 1.2
    ia, ib = (t.numpy() for t in TS.subset_indices(40, 30, 3, 10, 11))
    assert ia.shape == ib.shape == (3, 10) and all(len(set(r)) == 10 for r in ia) and all(len(set(r)) == 10 for r in ib)
    mean, std, vals = R.kid(real, fake, ia, ib)
    want = []
    for a, b in zip(ia, ib):
        k = lambda u, v: (u @ v / 6.0 + 1.0) ** 3               # noqa: E731
        xs, ys = real[a], fake[b]
        sxx = sum(k(xs[i], xs[j]) for i in range(10) for j in range(10) if i != j)
        syy = sum(k(ys[i], ys[j]) for i in range(10) for j in range(10) if i != j)
        sxy = sum(k(xs[i], ys[j]) for i in range(10) for j in range(10))
        want.append(sxx / 90 + syy / 90 - 2 * sxy / 100)
    assert np.abs(vals - want).max() <= 1e-12 * np.abs(want).max()
    assert abs(mean - np.mean(want)) <= 1e-12 and abs(std - np.std(want)) <= 1e-12
    # the same seed gives the same sets; another seed other sets
    again = TS.subset_indices(40, 30, 3, 10, 11)
    assert np.array_equal(again[0].numpy(), ia) and not np.array_equal(TS.subset_indices(40, 30, 3, 10, 12)[0].numpy(), ia)


# ================================================================================================ identities
def test_identities():
    x, y = rnd(12, 5, 8), rnd(9, 5, 9)
    for kind, kp, degree in ((R.RBF, R.params(R.RBF, [0.3, 0.6]), 0), (R.IMQ, R.params(R.IMQ, [0.3]), 0), (R.POLY, R.params(R.POLY, 0.2), 3)):
        assert abs(R.mmd2(kind, kp, degree, x, x.copy(), False)) <= 1e-13 * float(np.abs(R.kernel_matrix(kind, kp, degree, x, x)).max())
    # a = 0 turns the sums into pair counts
    zero = R.params(R.RBF, [0.0])
    assert np.array_equal(R.dense_sums(R.RBF, zero, 0, x, y), np.full(12, 9.0))
    assert np.array_equal(R.dense_sums(R.RBF, zero, 0, x, x, self0=0), np.full(12, 11.0))
    assert np.array_equal(R.dense_sums(R.RBF, zero, 0, x[3:], x, self0=3), np.full(9, 11.0))
    assert np.array_equal(R.dense_sums(R.RBF, zero, 0, x, x[4:], col0=4, self0=0), np.r_[np.full(4, 8.0), np.full(8, 7.0)])
    assert np.array_equal(R.ordered_parts(R.RBF, zero, 0, x, x, self0=0, P=1)[0], np.full(12, 11.0))
    # the permutation statistic of the identity split is the biased MMD^2
    kp = R.params(R.RBF, [0.3])
    signs = np.zeros((2, 21), dtype=bool)
    signs[0, :12] = True
    signs[1, 5:17] = True
    stats = R.permutation_stats(R.RBF, kp, 0, x, y, signs)
    want = R.mmd2(R.RBF, kp, 0, x, y, False)
    assert abs(stats[0] - want) <= 1e-13 and stats[1] == stats[0] and stats[2] != stats[0]
    assert R.p_value(np.array([1.0, 0.5, 1.0, 2.0])) == 3 / 4 and TS.p_value_of([1.0, 0.5, 1.0, 2.0]) == 3 / 4


def test_the_median_rule_is_the_lower_median():
    for vals in ([3.0, 1.0, 2.0], [4.0, 1.0, 3.0, 2.0], [5.0], [2.0, 2.0, 1.0, 7.0, 7.0, 9.0]):
        n = len(vals)
        want = sorted(vals)[(n + 1) // 2 - 1]
        assert R.lower_median(vals) == want
        assert float(torch.kthvalue(torch.tensor(vals), (n + 1) // 2).values) == want
    assert R.lower_median([4.0, 1.0, 3.0, 2.0]) == 2.0              # never the mean 2.5
    rows = rnd(6, 3, 10)                                            # 30 off-diagonal entries: even
    d = R.pair_values(R.RBF, rows, rows)
    off = np.sort(d[~np.eye(6, dtype=bool)])
    assert R.median_bandwidth(rows) == 1.0 / off[14]
    rows = rnd(2, 3, 10)
    assert R.median_bandwidth(rows) == 1.0 / R.pair_values(R.RBF, rows[:1], rows[1:])[0, 0]


def test_fmaf_emulation_is_exact():
    rs = np.random.RandomState(12)
    a = (rs.randn(4000) * 10.0 ** rs.randint(-3, 4, 4000)).astype(np.float32)
    b = (rs.randn(4000) * 10.0 ** rs.randint(-3, 4, 4000)).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1.0 + rs.randn(4000) * 1e-4)).astype(np.float32)     # heavy cancellation
    c[::3] = (rs.randn(len(c[::3])) * 100).astype(np.float32)
    got = R.fmaf32(a, b, c)
    for i in range(0, 4000, 7):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))                              # float(Fraction) rounds correctly to double: bracket in fp32
        cands = {float(lo), float(np.nextafter(lo, np.float32(np.inf))), float(np.nextafter(lo, np.float32(-np.inf)))}
        best = min(cands, key=lambda v: (abs(Fraction(v) - exact), int(np.float32(v).view(np.int32)) & 1))
        assert float(got[i]) == best, (i, a[i], b[i], c[i])


def test_the_fp32_pair_values_follow_the_16_block_rule():
    q, g = rnd(5, 37, 13), rnd(4, 37, 14)
    got = R.pair_values32(R.RBF, q, g)
    for i in range(5):
        for j in range(4):
            acc = 0.0
            for d0 in range(0, 37, 16):
                part = np.float32(0.0)
                for d in range(d0, min(d0 + 16, 37)):
                    dm = np.float32(q[i, d]) - np.float32(g[j, d])
                    part = R.fmaf32(np.array([dm]), np.array([dm]), np.array([part]))[0]
                acc += float(part)
            assert got[i, j] == np.float32(acc)
    assert np.abs(got - R.pair_values(R.RBF, q, g)).max() <= 37 * 2.0 ** -23 * R.pair_values(R.RBF, q, g).max()
    assert np.abs(R.pair_values32(R.POLY, q, g) - q @ g.T).max() <= 37 * 2.0 ** -23 * (np.abs(q) @ np.abs(g).T).max()


def test_partial_states_merge_exactly_on_integer_data():
    rs = np.random.RandomState(15)
    q, g = rs.randint(-8, 9, (70, 7)).astype(np.float64), rs.randint(-8, 9, (130, 7)).astype(np.float64)
    w = rs.randint(-3, 4, 130).astype(np.float64)
    kp = R.params(R.POLY, 1.0, 1.0)
    want = ((q.astype(np.int64) @ g.astype(np.int64).T + 1) ** 3 * w.astype(np.int64)[None, :]).sum(axis=1)
    assert np.array_equal(R.dense_sums(R.POLY, kp, 3, q, g, w), want.astype(np.float64))
    for P in (1, 2, 3, 64):
        part = R.ordered_parts(R.POLY, kp, 3, q, g, w, P=P)
        assert part.shape == (P, 70) and np.array_equal(R.finish_rows(part), want.astype(np.float64))
        if P == 64:
            assert not part[3:].any()                                # states that own no tile hold 0
    total = R.finish_total(want.astype(np.float64))
    assert total == float(want.sum())
    qw = rs.randint(-2, 3, 70).astype(np.float64)
    assert R.finish_total(want.astype(np.float64), qw) == float((want * qw.astype(np.int64)).sum())
    assert np.array_equal(R.finish_rows(R.ordered_parts(R.POLY, kp, 3, q, g, w, P=2), into=np.ones(70)), want + 1.0)


def test_the_kernel_order_follows_the_dense_form():
    q, g = R.case_rows(70, 130, 17)
    w = rnd(130, 1, 16)[:, 0]
    for name, n_scale, degree in R.KERNELS:
        kp = R.case_params(name, n_scale, degree, q, g)
        kind = R.KIND[name]
        tol, err = R.allowance(kind, kp, degree, q, g, w, self0=3)
        for P in (1, 3):
            got = R.finish_rows(R.ordered_parts(kind, kp, degree, q, g, w, self0=3, P=P))
            assert np.abs(got - R.dense_sums(kind, kp, degree, q, g, w, self0=3)).max() <= tol / 4.0, (name, P)
        assert 0.0 < err and tol < 1e-4 * np.abs(R.dense_sums(kind, kp, degree, q, g, w, self0=3)).max() + 1e-3


def test_special_values_reach_exactly_their_sums():
    q, g = R.case_rows(5, 70, 7)
    kp = R.params(R.RBF, [0.05])
    clean = R.finish_rows(R.ordered_parts(R.RBF, kp, 0, q, g, P=2))
    gn = g.copy()
    gn[66] = np.nan
    assert np.isnan(R.finish_rows(R.ordered_parts(R.RBF, kp, 0, q, gn, P=2))).all()           # every row reads column 66
    qn = q.copy()
    qn[2] = np.nan
    got = R.finish_rows(R.ordered_parts(R.RBF, kp, 0, qn, g, P=2))
    assert np.isnan(got[2]) and np.array_equal(np.delete(got, 2), np.delete(clean, 2))
    gi = g.copy()
    gi[1] = np.inf                                                                           # exp(-inf) = 0: the column drops out
    got = R.finish_rows(R.ordered_parts(R.RBF, kp, 0, q, gi, P=1))
    w = np.ones(70)
    w[1] = 0.0
    assert np.array_equal(got, R.finish_rows(R.ordered_parts(R.RBF, kp, 0, q, g, w, P=1)))
    # a self pair that holds a NaN is left out by predicate, not multiplied by 0
    x = g[:5].copy()
    pad = np.full((5, 7), np.nan)
    for i in range(5):
        pad[i] = x[i]
    got = R.dense_sums(R.RBF, R.params(R.RBF, [0.0]), 0, x, x, self0=0)
    assert np.array_equal(got, np.full(5, 4.0))
    assert np.isnan(R.finish_total(np.array([1.0, np.nan, 2.0])))


def test_analytic_prior_expectations_match_monte_carlo():
    rs = np.random.RandomState(17)
    D, n = 6, 200000
    kp = R.params(R.RBF, [0.05, 0.2, 0.6])
    x = rnd(3, D, 18)
    y, y2 = rs.randn(n, D), rs.randn(n, D)
    exy, eyy = R.rbf_prior_expectations(x, kp)
    for i in range(3):
        k = R.kernel_value(R.RBF, np.sum((x[i][None, :] - y) ** 2, axis=1), kp)
        assert abs(k.mean() - exy[i]) <= 5.0 * k.std() / np.sqrt(n), i
    k = R.kernel_value(R.RBF, np.sum((y - y2) ** 2, axis=1), kp)
    assert abs(k.mean() - eyy) <= 5.0 * k.std() / np.sqrt(n)
    t_exy, t_eyy = TS.rbf_prior_expectations(torch.from_numpy(x).float(), torch.from_numpy(kp))
    assert np.abs(t_exy.numpy() - exy).max() <= 1e-14 and abs(float(t_eyy) - eyy) <= 1e-14


# ================================================================================================ the GPU tests' inputs
@pytest.mark.parametrize("Q,N,D", R.SHAPES)
def test_the_inputs_of_the_gpu_value_tests_meet_their_conditions(Q, N, D):
    """every sum a tolerance is taken from has at least 8 effective terms at the median bandwidth (the two smallest shapes have 1 and 2
    terms in all: there the condition is that every term counts, i.e. as many effective terms as terms within 50 %)"""
    q, g = R.case_rows(Q, N, D)
    for name, n_scale, degree in R.KERNELS:
        kp = R.case_params(name, n_scale, degree, q, g)
        assert np.isfinite(kp).all() and (kp[:, 0] > 0).all()
        if name == "poly":
            continue                                                # signed terms: no effective count
        eff = R.effective_terms(R.KIND[name], kp, degree, q, g)
        assert eff.min() >= (8.0 if N >= 8 else 0.5 * N), (name, n_scale, eff.min())
        tol, err = R.allowance(R.KIND[name], kp, degree, q, g)
        assert tol < 1e-4 * R.dense_sums(R.KIND[name], kp, degree, q, g).min()


def test_the_inputs_of_the_gpu_permutation_test_meet_their_conditions():
    """at most 2 % of the permuted statistics lie within twice the allowance of the observed one; every row sum of the scan has at
    least 8 effective terms in absolute value"""
    x, y, signs = R.permutation_case()
    assert signs.shape == (R.PERM_B, R.PERM_N + R.PERM_M) and (signs.sum(axis=1) == R.PERM_N).all()
    kp = R.params(R.RBF, [R.median_bandwidth(np.concatenate([x, y]))])
    stats = R.permutation_stats(R.RBF, kp, 0, x, y, signs)
    tol = R.permutation_allowance(R.RBF, kp, 0, x, y)
    near = int(np.sum(np.abs(stats[1:] - stats[0]) <= 2.0 * tol))
    assert near <= 0.02 * R.PERM_B and tol < 1e-3 * abs(stats[0])
    z = np.concatenate([x, y])
    assert R.effective_terms(R.RBF, kp, 0, z, z).min() >= 8.0
    p = R.p_value(stats)
    assert 2.0 / (1 + R.PERM_B) <= p <= 1.0 - 2.0 / (1 + R.PERM_B), "the case should not sit at an end of the distribution"


# ================================================================================================ the entry points' refusals
P4 = C.c_void_p(4096)               # never dereferenced: nothing is launched
BIG = (1 << 63) - 1


def _scan(**kw):
    a = dict(kind=0, kparam=P4, n_scale=1, degree=3, q=P4, Q=5, q_stride=0, g=P4, g_w=P4, N=7, g_stride=0, w_stride=0, D=3, S=1, col0=0,
             self0=-1, P=1, part=P4)
    a.update(kw)
    return L.lib().sv_ksum_scan(a["kind"], a["kparam"], a["n_scale"], a["degree"], a["q"], a["Q"], a["q_stride"], a["g"], a["g_w"], a["N"],
                                a["g_stride"], a["w_stride"], a["D"], a["S"], a["col0"], a["self0"], a["P"], a["part"], None)


def _finish(**kw):
    a = dict(part=P4, S=1, P=1, Q=5, accumulate=0, row_sum=P4, q_w=None, w_stride=0, total=P4)
    a.update(kw)
    return L.lib().sv_ksum_finish(a["part"], a["S"], a["P"], a["Q"], a["accumulate"], a["row_sum"], a["q_w"], a["w_stride"], a["total"], None)


REFUSALS = [
    (_scan, "sv_ksum_scan", [
        (dict(kind=3), SV_E_ARG, b"kind"), (dict(kind=-1), SV_E_ARG, b"kind"), (dict(n_scale=0), SV_E_ARG, b"n_scale"),
        (dict(n_scale=9), SV_E_ARG, b"n_scale"), (dict(kind=1, n_scale=9), SV_E_ARG, b"n_scale"), (dict(kind=2, n_scale=2), SV_E_ARG, b"n_scale"),
        (dict(kind=2, degree=0), SV_E_ARG, b"degree"), (dict(kind=2, degree=9), SV_E_ARG, b"degree"), (dict(kparam=None), SV_E_ARG, b"NULL"),
        (dict(q=None), SV_E_ARG, b"NULL"), (dict(g=None), SV_E_ARG, b"NULL"), (dict(part=None), SV_E_ARG, b"NULL"),
        (dict(Q=0), SV_E_ARG, b"size"), (dict(N=-1), SV_E_ARG, b"size"), (dict(D=0), SV_E_ARG, b"size"), (dict(S=0), SV_E_ARG, b"S=0"),
        (dict(S=65536), SV_E_ARG, b"S=65536"), (dict(P=0), SV_E_ARG, b"P=0"), (dict(P=65), SV_E_ARG, b"P=65"),
        (dict(q_stride=14), SV_E_SHAPE, b"q_stride"), (dict(q_stride=-15), SV_E_SHAPE, b"q_stride"), (dict(g_stride=20), SV_E_SHAPE, b"g_stride"),
        (dict(w_stride=6), SV_E_SHAPE, b"w_stride"), (dict(w_stride=-7), SV_E_SHAPE, b"w_stride"),
        (dict(S=3, q_stride=BIG // 8), SV_E_SHAPE, b"overflow"), (dict(col0=-1), SV_E_ARG, b"col0"), (dict(self0=-2), SV_E_ARG, b"self0"),
        (dict(col0=BIG - 7), SV_E_SHAPE, b"overflows"), (dict(self0=BIG - 5), SV_E_SHAPE, b"overflows")]),
    (_finish, "sv_ksum_finish", [
        (dict(part=None), SV_E_ARG, b"NULL"), (dict(row_sum=None), SV_E_ARG, b"NULL"), (dict(Q=0), SV_E_ARG, b"size"),
        (dict(S=0), SV_E_ARG, b"S=0"), (dict(S=65536), SV_E_ARG, b"S=65536"), (dict(P=0), SV_E_ARG, b"P=0"), (dict(P=65), SV_E_ARG, b"P=65"),
        (dict(q_w=P4, total=None), SV_E_ARG, b"q_w"), (dict(q_w=P4, w_stride=4), SV_E_SHAPE, b"w_stride"),
        (dict(q_w=P4, w_stride=-5), SV_E_SHAPE, b"w_stride"), (dict(S=3, q_w=P4, w_stride=BIG // 8), SV_E_SHAPE, b"overflow")]),
]


@pytest.mark.parametrize("fn,name,cases", REFUSALS, ids=[r[1] for r in REFUSALS])
def test_entry_points_refuse_bad_arguments_before_any_launch(fn, name, cases):
    for kw, code, word in cases:
        assert fn(**kw) == code, (name, kw)
        err = L.lib().sv_last_error()
        assert word in err and name.encode() in err, (kw, err)


def test_entry_points_are_bound_and_exported():
    for name in ("sv_ksum_scan", "sv_ksum_finish"):
        assert name in L.EXPORTS and hasattr(L.lib(), name)
    assert L.lib().sv_version() == L.ABI_VERSION == 8
    for name in ("kernel_sums", "median_bandwidth", "mmd2", "witness", "kid", "permutation_test", "evaluate_two_sample",
                 "evaluate_prior_match", "evaluate_kid"):
        assert getattr(S, name) is getattr(TS, name)
    assert (L.KSUM_RBF, L.KSUM_IMQ, L.KSUM_POLY) == (R.RBF, R.IMQ, R.POLY) and TS.KINDS == R.KIND


# ================================================================================================ host logic
def test_python_layer_refuses_bad_arguments():
    x, y = torch.zeros(6, 3), torch.zeros(4, 3)
    for fn in (TS.kernel_sums, TS.mmd2, TS.permutation_test):
        name = fn.__name__
        with pytest.raises(ValueError, match=name + ".*matrix"):
            fn(torch.zeros(6), y)
        with pytest.raises(ValueError, match=name + ".*columns"):
            fn(x, torch.zeros(4, 2))
        with pytest.raises(ValueError, match=name + ".*kernel"):
            fn(x, y, kernel="laplace")
        with pytest.raises(ValueError, match=name + ".*degree"):
            fn(x, y, kernel="poly", gamma=1.0, degree=9)
        with pytest.raises(ValueError, match=name + ".*gamma"):
            fn(x, y, gamma="mean")
        with pytest.raises(ValueError, match=name + ".*poly"):
            fn(x, y, kernel="poly", gamma="median")
        with pytest.raises(ValueError, match=name + ".*bandwidths"):
            fn(x, y, gamma=[0.1] * 9)
        with pytest.raises(ValueError, match=name + ".*scales"):
            fn(x, y, gamma=1.0, scales=(1.0, -2.0))
        with pytest.raises(ValueError, match=name + ".*ONE bandwidth"):
            fn(x, y, gamma=[1.0, 2.0], scales=(1.0, 2.0))
    with pytest.raises(ValueError, match="kernel_sums.*weights"):
        TS.kernel_sums(x, y, gamma=1.0, weights=torch.zeros(5))
    with pytest.raises(ValueError, match="kernel_sums.*exclude_self_from"):
        TS.kernel_sums(x, y, gamma=1.0, exclude_self_from=-2)
    with pytest.raises(ValueError, match="mmd2.*two rows"):
        TS.mmd2(torch.zeros(1, 3), y, gamma=1.0)
    with pytest.raises(ValueError, match="witness.*columns"):
        TS.witness(x, y, torch.zeros(2, 4))
    with pytest.raises(ValueError, match="kid.*subsets"):
        TS.kid(x, y, subsets=0)
    with pytest.raises(ValueError, match="kid.*two rows"):
        TS.kid(x, torch.zeros(1, 3))
    with pytest.raises(ValueError, match="kid.*poly"):
        TS.kid(x, y, gamma="median")
    with pytest.raises(ValueError, match="permutation_test.*permutations"):
        TS.permutation_test(x, y, gamma=1.0, permutations=0)
    with pytest.raises(ValueError, match="permutation_test.*signs"):
        TS.permutation_test(x, y, gamma=1.0, signs=torch.zeros(3, 9, dtype=torch.bool))
    with pytest.raises(ValueError, match="permutation_test.*signs"):
        TS.permutation_test(x, y, gamma=1.0, signs=torch.zeros(3, 10))
    with pytest.raises(ValueError, match="median_bandwidth.*two rows"):
        TS.median_bandwidth(torch.zeros(1, 3))
    with pytest.raises(ValueError, match="median_bandwidth.*matrix"):
        TS.median_bandwidth(torch.zeros(3))
    for fn in (TS.evaluate_two_sample, TS.evaluate_prior_match, TS.evaluate_kid):
        with pytest.raises(TypeError, match=fn.__name__):
            fn(torch.nn.Linear(2, 2), [], []) if fn is TS.evaluate_two_sample else fn(torch.nn.Linear(2, 2), [])


def test_cpu_tensors_are_refused():
    x, y = torch.randn(6, 3), torch.randn(4, 3)
    for call in (lambda: TS.kernel_sums(x, y, gamma=1.0), lambda: TS.kernel_sums(x, y), lambda: TS.mmd2(x, y, gamma=0.5),
                 lambda: TS.witness(x, y, x, gamma=0.5), lambda: TS.kid(x, y, subsets=2, subset_size=3),
                 lambda: TS.permutation_test(x, y, gamma=0.5, permutations=3), lambda: TS.median_bandwidth(x, y)):
        with pytest.raises(L.ShotVaeHipError, match="MI355X"):
            call()


def test_split_weights_are_exact():
    member = torch.tensor([[True, True, False], [False, True, True]])
    w = TS.split_weights(member, 2, 1)
    assert w.dtype == torch.float32 and w.tolist() == [[1.0, 1.0, -2.0], [-2.0, 1.0, 1.0]]
    assert np.array_equal(R.split_weights(member.numpy(), 2, 1), w.numpy().astype(np.float64))
