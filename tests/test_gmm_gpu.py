"""Diagonal Gaussian mixtures on a real MI355X: sv_gmm_prepare, sv_gmm_estep, sv_gmm_accum, sv_gmm_finish and sv_gmm_sample through the C
ABI against the float64 restatement of tests/_gmm_ref.py (pinned to scikit-learn by tests/test_gmm_cpu.py), then the Python layer
(shot_vae_amd.mixture) and its joins in quality and calibration.

Integer-valued inputs are compared exactly.  Otherwise the allowances follow the project's 8x rule and are formed when the test runs,
never from a GPU result: R.allowance = 8 x the error of the fp32 numpy restatement of v and lse against float64 on the case's own inputs
(never less than 8 half ulps of fp32 at the largest value).  A responsibility r = exp(v - lse) <= 1 inherits |dr| <= r (|dv| + |dlse|)
plus expf's own rounding: RESP(tol) = 2 tol + 8 eps32, which also bounds |sum_k r - 1|.  An assignment is compared with float64 on the
rows whose float64 margin exceeds twice the allowance; on the separated blobs that must be every row.  The partial states are compared
bit for bit with the restatement's sums of the kernel's OWN r in the kernel's order (the issue allows 1 ulp of double; the order is
restated exactly, so equality is asked), and with the float64 restatement by |dS| <= RESP(tol) sum_i |x_id|^p.  Outputs carry guard
rows.  The measured figures are in DESIGN.md 4k."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import shot_vae_amd as S                                        # noqa: E402
from shot_vae_amd import _lib as L                              # noqa: E402
from shot_vae_amd import mixture as MX                          # noqa: E402
from tests import _gmm_ref as R                                 # noqa: E402
from tests import _knn_ref as KR                                # noqa: E402

GUARD = 3
EPS32 = float(np.finfo(np.float32).eps)


def dev():
    return torch.device("cuda:0")


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev())


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def ulp32(a):
    return np.spacing(np.abs(np.asarray(a, dtype=np.float32))).astype(np.float64)


def resp_tol(tol):
    return 2.0 * tol + 8.0 * EPS32


class Table:
    """a model on the device and its table from sv_gmm_prepare"""

    def __init__(self, logw, mean, var):
        self.K, self.D = mean.shape
        self.logw, self.mean, self.var = f32(logw), f32(mean), f32(var)
        self.ivar = torch.full((self.K + GUARD, self.D), -7.0, dtype=torch.float32, device=dev())
        self.cst = torch.full((self.K + GUARD,), -7.0, dtype=torch.float32, device=dev())
        self.cdf = torch.full((self.K + GUARD,), -7.0, dtype=torch.float32, device=dev())
        L.call("sv_gmm_prepare", p(self.logw), p(self.mean), p(self.var), self.K, self.D, p(self.ivar), p(self.cst), p(self.cdf), st())
        torch.cuda.synchronize()
        for t in (self.ivar, self.cst, self.cdf):
            assert bool((t[self.K:] == -7.0).all()), "sv_gmm_prepare wrote behind its outputs"


def estep(x, tab, cuts=None, want_assign=True, want_resp=True):
    """sv_gmm_estep over the rows cut at `cuts` -> (lse, assign, resp) numpy; the guard rows stay as they were"""
    N, K = x.shape[0], tab.K
    dx = f32(x)
    lse = torch.full((N + GUARD,), -7.0, dtype=torch.float32, device=dev())
    a = torch.full((N + GUARD,), -7, dtype=torch.int64, device=dev())
    r = torch.full((N + GUARD, K), -7.0, dtype=torch.float32, device=dev())
    edges = [0] + list(cuts or []) + [N]
    for lo, hi in zip(edges[:-1], edges[1:]):
        L.call("sv_gmm_estep", p(dx[lo:]), hi - lo, p(tab.ivar), p(tab.mean), p(tab.cst), K, tab.D, p(lse[lo:]),
               p(a[lo:]) if want_assign else None, p(r[lo:]) if want_resp else None, st())
    torch.cuda.synchronize()
    assert bool((lse[N:] == -7.0).all()) and bool((a[N:] == -7).all()) and bool((r[N:] == -7.0).all()), "sv_gmm_estep wrote behind its outputs"
    if not want_assign:
        assert bool((a == -7).all())
    if not want_resp:
        assert bool((r == -7.0).all())
    return lse[:N].cpu().numpy(), a[:N].cpu().numpy(), r[:N].cpu().numpy()


def accum(x, lse, tab, P, init=1, states=None, N=None):
    """sv_gmm_accum -> (sums float64 [P, stride], counts int64 [P, 2]) numpy; states: (sums, counts) device tensors to continue"""
    stride = R.state_stride(tab.K, tab.D)
    if states is None:
        states = (torch.full((P + 1, stride), -7.0, dtype=torch.float64, device=dev()), torch.full((P + 1, 2), -7, dtype=torch.int64, device=dev()))
    dx, dl = (x if torch.is_tensor(x) else f32(x)), (lse if torch.is_tensor(lse) else f32(lse))
    L.call("sv_gmm_accum", p(dx), p(dl), dx.shape[0] if N is None else N, p(tab.ivar), p(tab.mean), p(tab.cst), tab.K, tab.D, p(states[0]),
           p(states[1]), P, init, st())
    torch.cuda.synchronize()
    assert bool((states[0][P:] == -7.0).all()) and bool((states[1][P:] == -7).all()), "sv_gmm_accum wrote behind its states"
    return states[0][:P].cpu().numpy(), states[1][:P].cpu().numpy(), states


def data_for(N, K, D, seed, kind="spread"):
    """-> (x, logw, mean, var): rows about the components of a random mixture; "coincident": the components nearly coincide and their
    variances sit at the reg_covar floor"""
    rng = np.random.default_rng(seed)
    logw, mean, var = R.model(K, D, seed + 1)
    if kind == "coincident":
        mean = (mean[:1] + 1e-3 * rng.standard_normal((K, D))).astype(np.float32).astype(np.float64)
        var = np.full((K, D), np.float64(np.float32(1e-6)))
    which = rng.integers(0, K, N)
    x = mean[which] + np.sqrt(var[which]) * rng.standard_normal((N, D))
    return x.astype(np.float32).astype(np.float64), logw, mean, var


# ================================================================================================ sv_gmm_prepare
@pytest.mark.parametrize("K,D", [(1, 1), (2, 3), (17, 16), (65, 17), (257, 130), (1100, 5)])
def test_prepare_is_within_an_ulp_of_float64_and_the_cdf_ends_at_one(K, D):
    logw, mean, var = R.model(K, D, 8201)
    if K > 2:
        logw[[1, K - 1]] = -np.inf                          # a component of weight 0 inside, and at the end
    tab = Table(logw, mean, var)
    ivar, cst, cdf = R.prepare(logw, mean, var)
    got_i, got_c, got_f = host(tab.ivar[:K]), host(tab.cst[:K]), host(tab.cdf[:K])
    assert (np.abs(got_i - ivar) <= ulp32(ivar)).all()
    live = np.isfinite(cst)
    assert (np.abs(got_c[live] - cst[live]) <= ulp32(cst[live])).all() and np.isneginf(got_c[~live]).all()
    assert (np.abs(got_f - cdf) <= ulp32(cdf)).all() and (np.diff(got_f) >= 0).all()
    last = np.nonzero(np.exp(logw) > 0)[0][-1]
    assert got_f[last] == 1.0 and (got_f[last:] == 1.0).all() and (got_f[:last] <= 1.0).all()
    if K > 2:
        assert got_f[1] == got_f[0]


# ================================================================================================ sv_gmm_estep
ESTEP_SHAPES = [(1, 1, 1), (63, 2, 3), (65, 17, 16), (193, 65, 17), (65, 257, 130), (193, 2, 130), (63, 257, 1), (1, 17, 17), (193, 1, 3)]


@pytest.mark.parametrize("kind", ["spread", "coincident"])
@pytest.mark.parametrize("N,K,D", ESTEP_SHAPES)
def test_estep_matches_float64_by_the_8x_rule(N, K, D, kind):
    x, logw, mean, var = data_for(N, K, D, 8203, kind)
    tab = Table(logw, mean, var)
    ref_l, ref_a, ref_r = R.estep(x, logw, mean, var)
    tol = R.allowance(x, logw, mean, var)
    lse, a, r = estep(x, tab)
    err_l, err_r = float(np.abs(lse - ref_l).max()), float(np.abs(r - ref_r).max())
    err_s = float(np.abs(r.astype(np.float64).sum(axis=1) - 1.0).max())
    decided = R.margin(x, logw, mean, var) > 2.0 * tol
    print("FIG estep %s %s lse %.3e (%.3e) resp %.3e sum %.3e (%.3e) undecided %d" % ((N, K, D), kind, err_l, tol, err_r, err_s, resp_tol(tol),
                                                                                    int((~decided).sum())))
    assert err_l <= tol and err_r <= resp_tol(tol) and err_s <= resp_tol(tol)
    assert np.array_equal(a[decided], ref_a[decided]) and (a >= 0).all() and (a < K).all()
    assert (r[np.arange(N), a] == r.max(axis=1)).all()
    # the optional outputs change nothing, and rows cut into calls give the same bits
    assert np.array_equal(estep(x, tab, want_assign=False, want_resp=False)[0], lse)
    if N > 2:
        l2, a2, r2 = estep(x, tab, cuts=[1, N // 2])
        assert np.array_equal(l2, lse) and np.array_equal(a2, a) and np.array_equal(r2, r)


def test_estep_leaves_no_row_of_separated_blobs_undecided():
    for N, K, D in ((193, 3, 5), (130, 10, 128), (193, 65, 130)):
        x, cen, which = R.blobs(N, K, D, 8205)
        logw, mean, var = np.full(K, -math.log(K)), (cen + 0.125).astype(np.float32).astype(np.float64), np.full((K, D), 0.25)
        tab = Table(logw, mean, var)
        tol = R.allowance(x, logw, mean, var)
        margin = R.margin(x, logw, mean, var)
        assert (margin > 2.0 * tol).all(), "the reference leaves a row undecided"
        lse, a, _ = estep(x, tab, want_resp=False)
        print("FIG blobs %s lse %.3e (%.3e) least margin %.3e" % ((N, K, D), np.abs(lse - R.estep(x, logw, mean, var)[0]).max(), tol, margin.min()))
        assert np.array_equal(a, which) and np.array_equal(a, R.estep(x, logw, mean, var)[1])


@pytest.mark.parametrize("N,K,D", [(130, 66, 1), (65, 10, 17), (63, 258, 16)])
def test_assign_is_the_first_maximum_on_integer_rows_with_tied_components(N, K, D):
    rng = np.random.default_rng(8207)
    half = np.floor(rng.uniform(0, 2, (K // 2, D)))
    mean = np.concatenate([half, half])                      # every component twice: exact ties, K / 2 apart
    x = np.floor(rng.uniform(0, 2, (N, D)))
    logw, var = np.full(K, -math.log(K)), np.ones((K, D))
    ref_a = R.estep(x, logw, mean, var)[1]
    v = R.pair_values(x, logw, mean, var)
    assert ((v == v.max(axis=1, keepdims=True)).sum(axis=1) > 1).all() and (ref_a < K // 2).all()
    lse, a, r = estep(x, Table(logw, mean, var))
    assert np.array_equal(a, ref_a)
    assert np.array_equal(r[:, :K // 2], r[:, K // 2:])


def test_estep_rules_of_special_rows_and_components():
    N, K, D = 70, 5, 19
    x, logw, mean, var = data_for(N, K, D, 8209)
    x[3, 18], x[64, 0], x[65, 7] = np.nan, np.inf, -np.inf
    x[9] = 100.0                                             # a far outlier: every v is about -1e5
    logw[2] = -np.inf
    tab = Table(logw, mean, var)
    lse, a, r = estep(x, tab)
    bad = [3, 64, 65]
    ok = np.setdiff1d(np.arange(N), bad)
    assert np.isnan(lse[bad]).all() and (a[bad] == -1).all() and np.isnan(r[bad]).all()
    assert np.isfinite(lse[ok]).all() and np.isfinite(r[ok]).all() and (a[ok] >= 0).all()
    assert (r[ok][:, 2] == 0).all() and (a[ok] != 2).all()
    ref_l, ref_a, ref_r = R.estep(x, logw, mean, var)
    tol = R.allowance(np.delete(x, 9, axis=0), logw, mean, var)
    rows = np.setdiff1d(ok, [9])
    assert np.abs(lse[rows] - ref_l[rows]).max() <= tol and np.array_equal(a[rows][R.margin(x, logw, mean, var)[rows] > 2 * tol],
                                                                         ref_a[rows][R.margin(x, logw, mean, var)[rows] > 2 * tol])
    out_tol = R.allowance(x[9:10], logw, mean, var)
    print("FIG outlier lse %.6e err %.3e (%.3e) sum %.3e" % (lse[9], abs(lse[9] - ref_l[9]), out_tol, abs(r[9].astype(np.float64).sum() - 1)))
    assert np.isfinite(r[9]).all() and abs(lse[9] - ref_l[9]) <= out_tol and abs(r[9].astype(np.float64).sum() - 1.0) <= resp_tol(out_tol)
    # every component of weight 0: lse = -inf, no assignment
    none = Table(np.full(K, -np.inf), mean, var)
    lse, a, _ = estep(x[:5], none, want_resp=False)
    assert np.isneginf(lse[[0, 1, 2, 4]]).all() and np.isnan(lse[3]) and (a == -1).all()


# ================================================================================================ sv_gmm_accum
def test_accum_forms_the_responsibilities_of_the_estep_bit_for_bit():
    for N, K, D in ((9, 5, 19), (6, 70, 33)):
        x, logw, mean, var = data_for(N, K, D, 8211)
        tab = Table(logw, mean, var)
        lse, _, r = estep(x, tab)
        for i in range(N):
            sums, counts, _ = accum(x[i:i + 1], lse[i:i + 1], tab, 1)
            body = sums[0, :-1].reshape(K, 2 * D + 1)
            assert np.array_equal(body[:, 0], r[i].astype(np.float64)), (N, K, D, i)
            assert counts.tolist() == [[1, 0]] and sums[0, -1] == np.float64(lse[i])


@pytest.mark.parametrize("N,K,D,P", [(453, 3, 5, 1), (453, 10, 33, 3), (4096, 17, 16, 64), (453, 65, 130, 3), (64 * 64, 2, 3, 64)])
def test_accum_sums_are_exact_on_integer_rows_with_one_hot_responsibilities(N, K, D, P):
    rng = np.random.default_rng(8213)
    mean = 16.0 * np.arange(K)[:, None] + np.floor(rng.uniform(0, 4, (K, D)))
    which = rng.integers(0, K, N)
    x = mean[which] + np.floor(rng.uniform(-1, 2, (N, D)))
    logw, var = np.full(K, -math.log(K)), np.full((K, D), 1.0 / 64)
    tab = Table(logw, mean, var)
    lse, a, r = estep(x, tab)
    assert np.array_equal(a, which) and np.array_equal(r, np.eye(K, dtype=np.float32)[which])
    sums, counts, _ = accum(x, lse, tab, P)
    want, wc = R.accum(x, np.eye(K)[which], lse.astype(np.float64), P)
    assert np.array_equal(sums, want) and np.array_equal(counts, wc)
    body = R.merge(sums)[:-1].reshape(K, 2 * D + 1)
    assert np.array_equal(body[:, 0], np.bincount(which, minlength=K).astype(np.float64))
    assert np.array_equal(body[:, 1:D + 1], np.eye(K)[which].T @ x) and np.array_equal(body[:, D + 1:], np.eye(K)[which].T @ (x * x))


@pytest.mark.parametrize("N,K,D,P", [(453, 3, 5, 1), (453, 17, 33, 3), (4096, 10, 16, 64), (453, 65, 130, 3), (200, 130, 17, 3)])
def test_accum_states_hold_the_kernels_own_sums_and_follow_the_cut_rules(N, K, D, P):
    x, logw, mean, var = data_for(N, K, D, 8215)
    x[5, 0], x[N - 2, D - 1] = np.nan, np.inf
    tab = Table(logw, mean, var)
    lse, _, r = estep(x, tab)
    dx, dl = f32(x), f32(lse)
    sums, counts, states = accum(dx, dl, tab, P)
    # (1) the kernel's own r, in the kernel's order: the same bits
    want, wc = R.accum(np.where(np.isfinite(x), x, 0.0), np.where(np.isfinite(r), r, 0.0), lse, P)
    assert np.array_equal(counts, wc) and int(counts[:, 1].sum()) == 2 and int(counts.sum()) == N
    ulps = np.abs(sums - want) / np.spacing(np.maximum(np.abs(want), np.finfo(np.float64).tiny))
    print("FIG accum %s against its own r: %.1f ulp of double" % ((N, K, D, P), ulps.max()))
    assert np.array_equal(sums, want)
    # (2) the float64 restatement, by the 8x rule
    ok = np.isfinite(x).all(axis=1)
    tol = resp_tol(R.allowance(x[ok], logw, mean, var))
    ref_l, _, ref_r = R.estep(x, logw, mean, var)
    ref = R.merge(R.accum(np.where(np.isfinite(x), x, 0.0), np.where(np.isfinite(ref_r), ref_r, 0.0), ref_l, P)[0])[:-1].reshape(K, 2 * D + 1)
    got = R.merge(sums)[:-1].reshape(K, 2 * D + 1)
    ax = np.abs(x[ok])
    bound = np.concatenate([[float(ok.sum())], ax.sum(axis=0), (ax * ax).sum(axis=0)]) * tol
    err = np.abs(got - ref)
    print("FIG accum %s against float64: r-sum %.3e (%.3e) S1 %.3e (%.3e) S2 %.3e (%.3e)"
          % ((N, K, D, P), err[:, 0].max(), bound[0], err[:, 1:D + 1].max(), bound[1:D + 1].min(), err[:, D + 1:].max(), bound[D + 1:].min()))
    assert (err <= bound[None, :]).all()
    # (3) a repeat gives the same bits; the cuts at multiples of 64 P continue to the bits of the one call
    assert np.array_equal(accum(dx, dl, tab, P)[0], sums)
    cut = 64 * P * max(1, (N // (64 * P)) // 2)
    if cut < N:
        _, _, part = accum(dx[:cut], dl[:cut], tab, P)
        s2, c2, _ = accum(dx[cut:], dl[cut:], tab, P, init=0, states=part)
        assert np.array_equal(s2, sums) and np.array_equal(c2, counts)
    if P == 1:
        _, _, part = accum(dx[:64], dl[:64], tab, 1)
        _, _, part = accum(dx[64:320], dl[64:320], tab, 1, init=0, states=part)
        s3, c3, _ = accum(dx[320:], dl[320:], tab, 1, init=0, states=part)
        assert np.array_equal(s3, sums) and np.array_equal(c3, counts)
    # (4) init = 0 continues: the same rows again double every integer count
    s4, c4, _ = accum(dx, dl, tab, P, init=0, states=states)
    assert np.array_equal(c4, 2 * counts)


# ================================================================================================ sv_gmm_finish
def finish(sums, counts, P, K, D, reg, logw, mean, var):
    """sv_gmm_finish in place on a fresh copy of the model -> dict of numpy arrays"""
    t = dict(logw=f32(logw), mean=f32(mean), var=f32(var))
    for name, shape in (("ivar", (K, D)), ("cst", (K,)), ("cdf", (K,)), ("stats", (4,))):
        t[name] = torch.full(shape, -7.0, dtype=torch.float32, device=dev())
    ds, dc = torch.from_numpy(sums).to(dev()), torch.from_numpy(counts).to(dev())
    L.call("sv_gmm_finish", p(ds), p(dc), P, K, D, float(reg), p(t["logw"]), p(t["mean"]), p(t["var"]), p(t["ivar"]), p(t["cst"]), p(t["cdf"]),
           p(t["stats"]), st())
    torch.cuda.synchronize()
    return {k: host(v) for k, v in t.items()}


@pytest.mark.parametrize("N,K,D,P", [(453, 3, 5, 1), (453, 17, 33, 3), (4096, 10, 16, 64), (300, 257, 130, 2)])
def test_finish_is_within_an_ulp_of_the_float64_m_step(N, K, D, P):
    x, logw, mean, var = data_for(N, K, D, 8217)
    x[7, 0] = np.nan
    tab = Table(logw, mean, var)
    lse, _, _ = estep(x, tab, want_resp=False)
    sums, counts, _ = accum(x, lse, tab, P)
    if K > 2:
        for q in range(P):
            sums[q, :-1].reshape(K, 2 * D + 1)[1, :] = 0.0   # an empty component
    got = finish(sums, counts, P, K, D, 1e-6, logw, mean, var)
    lw, m, v, stats = R.finish(sums, counts, K, D, 1e-6, logw, mean, var)
    live = np.isfinite(lw)
    assert (np.abs(got["mean"] - m) <= ulp32(m)).all() and (np.abs(got["var"] - v) <= ulp32(v)).all()
    assert (np.abs(got["logw"][live] - lw[live]) <= ulp32(lw[live])).all() and np.isneginf(got["logw"][~live]).all()
    if K > 2:
        assert not live[1] and np.array_equal(got["mean"][1], np.float32(mean[1]).astype(np.float64)) and np.array_equal(
            got["var"][1], np.float32(var[1]).astype(np.float64))
    # the table: sv_gmm_prepare's, from the fp32 model that was written
    ivar, cst, cdf = R.prepare(got["logw"], got["mean"], got["var"])
    assert (np.abs(got["ivar"] - ivar) <= ulp32(ivar)).all() and (np.abs(got["cst"][live] - cst[live]) <= ulp32(cst[live])).all()
    assert (np.abs(got["cdf"] - cdf) <= ulp32(cdf)).all() and got["cdf"][np.nonzero(live)[0][-1]] == 1.0
    tab2 = Table(got["logw"], got["mean"], got["var"])
    for name, t in (("ivar", tab2.ivar), ("cst", tab2.cst), ("cdf", tab2.cdf)):
        assert np.array_equal(got[name], host(t[:K]), equal_nan=True), name
    want = np.array([stats[0], stats[1], stats[2], np.float32(v[live]).min()])
    assert (np.abs(got["stats"] - want) <= ulp32(want)).all() and got["stats"][1] == N - 1 and got["stats"][2] == 1


def test_finish_on_identical_rows_gives_reg_covar_up_to_the_subtraction():
    """N identical rows c, one component: S1 / n = c (1 - e), S2 / n = c^2 (1 - e) with e = 10 eps / N from scikit-learn's n_k, so
    S2 / n - mean^2 = c^2 e (1 - e) plus the roundings of the two quotients, the square and the difference, each at most c^2 2^-53:
    |var - reg_covar| <= c^2 (10 eps / N + 4 * 2^-53), then one rounding to fp32"""
    N, D, reg = 300, 7, 1e-3
    c = np.float32(np.random.default_rng(8219).uniform(-3, 3, D)).astype(np.float64)
    x = np.tile(c, (N, 1))
    tab = Table(np.zeros(1), np.zeros((1, D)), np.ones((1, D)))
    lse, _, _ = estep(x, tab, want_resp=False)
    sums, counts, _ = accum(x, lse, tab, 2)
    got = finish(sums, counts, 2, 1, D, reg, np.zeros(1), np.zeros((1, D)), np.ones((1, D)))
    slack = c * c * (10 * np.finfo(np.float64).eps / N + 4 * 2.0 ** -53)
    print("FIG identical rows: |var - reg_covar| %.3e, allowed %.3e" % (np.abs(got["var"][0] - reg).max(), (slack + ulp32(reg)).max()))
    assert (np.abs(got["var"][0] - reg) <= slack + ulp32(reg)).all()
    assert (np.abs(got["mean"][0] - c) <= ulp32(c)).all() and got["logw"][0] == 0.0 and got["cdf"][0] == 1.0
    assert abs(got["stats"][3] - got["var"].min()) == 0.0


# ================================================================================================ sv_gmm_sample
def sample(tab, key, row0, B, want_comp=True):
    z = torch.full((B + GUARD, tab.D), -7.0, dtype=torch.float32, device=dev())
    c = torch.full((B + GUARD,), -7, dtype=torch.int64, device=dev())
    dk = torch.tensor([key], dtype=torch.int64, device=dev())
    L.call("sv_gmm_sample", p(tab.mean), p(tab.var), p(tab.cdf), tab.K, tab.D, p(dk), row0, B, p(z), p(c) if want_comp else None, st())
    torch.cuda.synchronize()
    assert bool((z[B:] == -7.0).all()) and bool((c[B:] == -7).all()), "sv_gmm_sample wrote behind its outputs"
    return host(z[:B]), c[:B].cpu().numpy()


@pytest.mark.parametrize("K,D,B,row0", [(1, 1, 5, 0), (3, 5, 130, 7), (17, 130, 65, 2 ** 33 + 5), (300, 3, 257, 0)])
def test_sample_is_the_numpy_restatement_and_split_independent(K, D, B, row0):
    """components exactly; z within one fp32 rounding of sqrtf(var) n and of the sum, plus the device's own error in the normal (logf,
    cosf, sinf of a few ulp: |dn| <= 2e-6 (1 + |n|), the bound the stream's other tests use is of this size)"""
    logw, mean, var = R.model(K, D, 8221)
    if K > 2:
        logw[1] = -np.inf
    tab = Table(logw, mean, var)
    key = -0x123456789ABCDEF
    z, c = sample(tab, key, row0, B)
    ref_z, ref_c = R.sample(key, row0, B, np.float32(mean), np.float32(var), host(tab.cdf[:K]))
    assert np.array_equal(c, ref_c) and (K <= 2 or 1 not in c)
    n = R.sample_normals(key, row0, B, D)
    sd = np.sqrt(np.float32(var).astype(np.float64))[c]
    tol = sd * 2e-6 * (1.0 + np.abs(n)) + ulp32(sd * n) + ulp32(ref_z)
    print("FIG sample %s err %.3e (least allowance %.3e)" % ((K, D, B), np.abs(z - ref_z).max(), tol.min()))
    assert (np.abs(z - ref_z) <= tol).all()
    cutz, cutc = zip(*(sample(tab, key, row0 + lo, hi - lo) for lo, hi in ((0, 1), (1, B // 2), (B // 2, B)) if hi > lo))
    assert np.array_equal(np.concatenate(cutz), z) and np.array_equal(np.concatenate(cutc), c)
    assert np.array_equal(sample(tab, key, row0, B, want_comp=False)[0], z)
    assert not np.array_equal(sample(tab, key + 1, row0, B)[0], z)


def test_sample_frequencies_stay_inside_a_binomial_bound():
    """2^16 rows: the count of component k is Binomial(n, w_k) if the uniforms are; 6 standard deviations (two-sided 2e-9 per component)
    around n w_k, plus one row for the fp32 rounding of each cdf edge (n 2^-24 < 1 row)"""
    B = 1 << 16
    w = np.array([0.4, 0.0, 0.25, 0.2, 0.1, 0.05, 0.0])
    with np.errstate(divide="ignore"):
        tab = Table(np.log(w), np.zeros((7, 2)), np.ones((7, 2)))
    _, c = sample(tab, 99, 0, B)
    count = np.bincount(c, minlength=7)
    bound = 6.0 * np.sqrt(B * w * (1 - w)) + 2.0
    print("FIG frequencies", count.tolist(), "expected", (B * w).tolist(), "bound", np.round(bound, 1).tolist())
    assert (np.abs(count - B * w) <= bound).all() and count[1] == 0 and count[6] == 0


# ================================================================================================ GaussianMixture
def em_step32(x, logw, mean, var, reg):
    """the fp32 restatement of one iteration: the E-step in float32, the M-step of those responsibilities, parameters rounded to fp32"""
    lse, _, resp = R.estep(x, logw, mean, var, np.float32)
    _, lw, m, v = R.mstep(x, resp.astype(np.float64), reg)
    return tuple(np.float32(a).astype(np.float64) for a in (lw, m, v)) + (float(lse.astype(np.float64).mean()),)


def start_of(x, K, seed):
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.5, 1.5, K)
    f = lambda a: np.float32(a).astype(np.float64)          # noqa: E731
    return w / w.sum(), f(x[rng.choice(len(x), K, replace=False)] + 0.1), f(rng.uniform(0.5, 2.0, (K, x.shape[1])))


def mixture_at(K, D, w, m, v, reg=1e-6):
    gm = S.GaussianMixture(K, D, reg_covar=reg)
    return gm.set_parameters(torch.from_numpy(np.asarray(w, dtype=np.float64)).to(dev()), f32(m), f32(v))


def test_step_is_the_three_calls_by_hand_and_a_replayed_graph():
    N, K, D = 700, 5, 19
    x, _, _ = R.blobs(N, K, D, 8223, spread=1.0)
    w, m, v = start_of(x, K, 8224)
    gm = mixture_at(K, D, w, m, v)
    dx = f32(x)
    stats = gm.step(dx).clone()
    # by hand
    tab = Table(np.log(w), m, v)
    assert torch.equal(tab.cst[:K], mixture_at(K, D, w, m, v)._ready("test")[1])
    lse, _, _ = estep(x, tab, want_resp=False)
    P = MX._partials(K, D, N)
    sums, counts, _ = accum(x, lse, tab, P)
    got = finish(sums, counts, P, K, D, 1e-6, np.float32(np.log(w)), m, v)
    assert np.array_equal(host(gm.logw), got["logw"]) and np.array_equal(host(gm.mean), got["mean"]) and np.array_equal(host(gm.var), got["var"])
    assert np.array_equal(host(stats), got["stats"]) and np.array_equal(host(gm._table[1]), got["cst"])
    # a graph captured on one set of rows, replayed on another
    buf = dx.clone()
    g2 = mixture_at(K, D, w, m, v)
    g2.step(buf)                                            # (allocates the workspace)
    g2.set_parameters(torch.from_numpy(w).to(dev()), f32(m), f32(v))
    start = [t.clone() for t in (g2.logw, g2.mean, g2.var)]
    g2._ready("test")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            g2.step(buf)
    torch.cuda.current_stream().wait_stream(side)
    x2, _, _ = R.blobs(N, K, D, 8225, spread=1.0)
    for rows in (x2, x):
        buf.copy_(f32(rows))
        for t, s0 in zip((g2.logw, g2.mean, g2.var), start):
            t.copy_(s0)
        L.call("sv_gmm_prepare", p(g2.logw), p(g2.mean), p(g2.var), K, D, p(g2._table[0]), p(g2._table[1]), p(g2._table[2]), st())
        graph.replay()
        torch.cuda.synchronize()
        eager = mixture_at(K, D, w, m, v)
        est = eager.step(f32(rows))
        assert torch.equal(g2.mean, eager.mean) and torch.equal(g2.var, eager.var) and torch.equal(g2.logw, eager.logw)
        assert torch.equal(g2.stats, est)
    assert torch.equal(g2.mean, gm.mean)


def test_five_iterations_follow_scikit_learn_from_the_same_start():
    sk = pytest.importorskip("sklearn.mixture")
    import warnings
    N, K, D = 600, 3, 5
    x, _, _ = R.blobs(N, K, D, 8227, spread=0.5)
    w, m, v = start_of(x, K, 8228)
    gm = mixture_at(K, D, w, m, v)
    dx = f32(x)
    ref = r32 = (np.log(w), m, v)
    for it in range(5):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            skm = sk.GaussianMixture(K, covariance_type="diag", weights_init=np.exp(ref[0]) / np.exp(ref[0]).sum(), means_init=ref[1],
                                     precisions_init=1.0 / ref[2], max_iter=1, tol=0.0, reg_covar=1e-6).fit(x)
        r32 = em_step32(x, *r32[:3], 1e-6)                  # the fp32 restatement follows its own iterates, as the kernels do
        ref = R.em_step(x, *ref[:3], 1e-6)
        assert np.abs(ref[1] - skm.means_).max() <= 1e-10 and np.abs(ref[2] - skm.covariances_).max() <= 1e-10
        assert abs(ref[3] - skm.lower_bound_) <= 1e-10
        stats = host(gm.step(dx))
        got = (host(gm.logw), host(gm.mean), host(gm.var), stats[0])
        for name, a, b, c in zip(("logw", "mean", "var", "bound"), got, ref, r32):
            tol = 8.0 * max(float(np.abs(np.asarray(c) - np.asarray(b)).max()), R.half_ulp32(b))
            err = float(np.abs(np.asarray(a) - np.asarray(b)).max())
            print("FIG iterate %d %s err %.3e (%.3e)" % (it + 1, name, err, tol))
            assert err <= tol, (it, name)


def test_fit_recovers_the_blobs_and_n_init_keeps_the_higher_bound_without_host_reads(monkeypatch):
    N, K, D = 900, 3, 6
    x, cen, which = R.blobs(N, K, D, 8229, spread=0.5)
    dx = f32(x)
    gm = S.GaussianMixture(K, D, seed=3).fit(dx, max_iter=50, tol=1e-4)
    assert gm.converged_ and 1 <= gm.n_iter_ < 50
    mean = host(gm.mean)
    order = [int(np.abs(mean - c).sum(axis=1).argmin()) for c in cen]
    assert sorted(order) == [0, 1, 2] and np.abs(mean[order] - cen).max() <= 6 * 0.5 / math.sqrt(N / K)
    assert np.abs(host(gm.var) - 0.25).max() <= 0.1 and np.abs(host(gm.weights) - 1 / 3).max() <= 1e-3
    pred = gm.predict(dx).cpu().numpy()
    assert np.array_equal(np.array(order)[which], pred)
    proba = host(gm.predict_proba(dx))
    assert np.abs(proba.sum(axis=1) - 1.0).max() <= 1e-5 and np.array_equal(proba.argmax(axis=1), pred)
    total = float(gm.score(dx))
    assert abs(total / N - float(gm.lower_bound_)) <= 1e-3
    assert abs(float(gm.bic(dx)) - (-2 * total + MX.n_parameters(K, D) * math.log(N))) <= 1e-6 * abs(total)
    assert abs(float(gm.aic(dx)) - (-2 * total + 2 * MX.n_parameters(K, D))) <= 1e-6 * abs(total)

    # n_init: random starts differ; the run with the highest bound is kept, chosen on the device
    x2, _, _ = R.blobs(600, 6, 4, 8231, spread=1.0)
    d2 = f32(x2)
    runs, gen = [], torch.Generator().manual_seed(11)
    for _ in range(4):
        one = S.GaussianMixture(6, 4, init="random", seed=11)
        one.reset(d2, gen)
        for _ in range(6):
            bound = float(one.step(d2)[0])
        runs.append((bound, one.mean.clone()))
    reads = []
    for name in ("cpu", "item", "tolist"):
        monkeypatch.setattr(torch.Tensor, name, (lambda real: lambda self, *a, **k: (reads.append(1), real(self, *a, **k))[1])(getattr(torch.Tensor, name)))
    best = S.GaussianMixture(6, 4, init="random", seed=11).fit(d2, max_iter=6, tol=None, n_init=4)
    monkeypatch.undo()
    assert not reads, "fit(tol=None) read from the device"
    top = max(range(4), key=lambda i: runs[i][0])
    assert len({r[0] for r in runs}) > 1, "the case cannot tell the runs apart"
    assert torch.equal(best.mean, runs[top][1]) and float(best.lower_bound_) == np.float32(runs[top][0])
    assert best.n_iter_ == 6 and best.converged_ is False


def test_state_dict_round_trip_on_the_device():
    logw, mean, var = R.model(4, 9, 8233)
    gm = mixture_at(4, 9, np.exp(logw), mean, var)
    x = f32(data_for(50, 4, 9, 8233)[0])
    sd = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in gm.state_dict().items()}
    other = S.GaussianMixture(4, 9).load_state_dict(sd, device=dev())
    assert torch.equal(other.score_samples(x), gm.score_samples(x)) and torch.equal(other.sample(7, 5), gm.sample(7, 5))
    z, c = gm.sample(7, 5, row0=3, return_component=True)
    assert torch.equal(z[:4], gm.sample(4, torch.tensor([5], device=dev()), row0=3)) and c.dtype == torch.int64


# ================================================================================================ the models
def batches_of(images, labels, B):
    return [(images[i:i + B], labels[i:i + B]) for i in range(0, images.shape[0], B)]


@pytest.mark.parametrize("kind", KR.EVAL_KINDS)
def test_evaluate_mixture_on_both_model_families(kind):
    from tests.test_cluster_gpu import eval_model
    model = eval_model(kind)
    gi, gl, ti, tl = (t.to(dev()) for t in KR.eval_images(kind))
    args = dict(k=3, seed=2, max_iter=4, tol=None, reg_covar=1e-4)
    res = S.evaluate_mixture(model, batches_of(gi, gl, 16), batches_of(ti, tl, 16), **args)
    gm = res["mixture"]
    mu_f = torch.cat([S.encode_posterior(model, x)[0] for x, _ in batches_of(gi, gl, 16)])
    mu_t = torch.cat([S.encode_posterior(model, x)[0] for x, _ in batches_of(ti, tl, 16)])
    D = mu_f.shape[1]
    params = (host(gm.logw), host(gm.mean), host(gm.var))
    for name, mu in (("fit", mu_f), ("test", mu_t)):
        ref = R.estep(host(mu), *params)[0]
        tol = R.allowance(host(mu), *params)
        print("FIG evaluate_mixture %s ll_%s %.6e err %.3e (%.3e) prior %.6e" % (kind, name, res["ll_" + name], abs(res["ll_" + name] - ref.mean()),
                                                                              tol, res["prior_ll_" + name]))
        assert abs(res["ll_" + name] - ref.mean()) <= tol
        prior = -0.5 * (D * math.log(2 * math.pi) + (host(mu) ** 2).sum(axis=1).mean())
        assert abs(res["prior_ll_" + name] - prior) <= 1e-9 * abs(prior)
        pred = gm.predict(mu).cpu().numpy()
        label = (gl if name == "fit" else tl).cpu().numpy()
        table = np.zeros((KR.EVAL_CLASSES, 3), dtype=np.int64)
        np.add.at(table, (label, pred), 1)
        want = S.partition_metrics(table)
        assert all(abs(res["partition_" + name][q] - want[q]) <= 1e-12 for q in ("accuracy", "nmi", "ari", "purity"))
    n, npar = KR.EVAL_GALLERY, MX.n_parameters(3, D)
    assert res["n_fit"] == n and res["n_test"] == KR.EVAL_TEST and res["n_parameters"] == npar
    assert abs(res["bic"] - (-2 * res["ll_fit"] * n + npar * math.log(n))) <= 1e-9 * abs(res["bic"])
    assert abs(res["aic"] - (-2 * res["ll_fit"] * n + 2 * npar)) <= 1e-9 * abs(res["aic"])
    # re-batched: the rows are gathered before anything is fitted, so the same rows give the same bits.  (An encoder whose own bits
    # depend on its batch size hands over other rows: then each result is held to its own reference, as above.)
    other = S.evaluate_mixture(model, batches_of(gi, gl, 12), batches_of(ti, tl, 48), **args)
    again = torch.cat([S.encode_posterior(model, x)[0] for x, _ in batches_of(gi, gl, 12)])
    same = torch.equal(again, mu_f) and torch.equal(S.encode_posterior(model, ti)[0], mu_t)
    print("FIG evaluate_mixture %s: the encoder's rows %s on the batch size" % (kind, "do not depend" if same else "DEPEND"))
    if same:
        assert torch.equal(other["mixture"].mean, gm.mean) and all(other[q] == res[q] for q in ("ll_fit", "ll_test", "bic", "aic", "prior_ll_fit"))
    else:
        om = other["mixture"]
        ref = R.estep(host(again), host(om.logw), host(om.mean), host(om.var))[0]
        assert abs(other["ll_fit"] - ref.mean()) <= R.allowance(host(again), host(om.logw), host(om.mean), host(om.var))
    twice = S.evaluate_mixture(model, batches_of(gi, gl, 16), batches_of(ti, tl, 16), **args)
    assert torch.equal(twice["mixture"].mean, gm.mean) and all(twice[q] == res[q] for q in ("ll_fit", "ll_test", "bic", "aic", "prior_ll_fit"))
    bare = S.evaluate_mixture(model, [gi[:40], gi[40:]], **args)
    assert bare["partition_fit"] is None and bare["ll_test"] is None and bare["ll_fit"] == res["ll_fit"]


@pytest.mark.parametrize("kind", KR.EVAL_KINDS)
def test_generation_and_detection_from_a_mixture(kind):
    from tests.test_cluster_gpu import eval_model
    model = eval_model(kind)
    gi, gl, ti, tl = (t.to(dev()) for t in KR.eval_images(kind))
    mu = S.encode_posterior(model, gi)[0]
    gm = S.GaussianMixture(3, mu.shape[1], reg_covar=1e-4, seed=1).fit(mu, max_iter=3, tol=None)
    labels = tl[:20].contiguous()
    img = S.generate_from_mixture(model, gm, labels, key=5, row0=2)
    z = gm.sample(20, 5, row0=2)
    if kind == "svhn":
        hot = torch.nn.functional.one_hot(labels, KR.EVAL_CLASSES).float()
        with torch.no_grad():
            want = model.decode(torch.cat([z, hot], dim=1))
    else:
        want = model.decode(z, labels, sigmoid=True)
    assert torch.equal(img, want) and img.shape[0] == 20 and bool(torch.isfinite(img).all())
    parts = torch.cat([S.generate_from_mixture(model, gm, labels[:7], key=5, row0=2), S.generate_from_mixture(model, gm, labels[7:], key=5, row0=9)])
    assert torch.equal(parts, img)
    # evaluate_generation: the new source runs, is independent of the batching, and differs from the prior's samples; the old calls give
    # what they gave with or without the new argument
    real = ti
    a = S.evaluate_generation(model, batches_of(real, tl, 16), source="mixture", mixture=gm, key=4, k=3)
    b = S.evaluate_generation(model, batches_of(real, tl, 12), source="mixture", mixture=gm, key=4, k=3)
    old = S.evaluate_generation(model, batches_of(real, tl, 16), key=4, k=3)
    old2 = S.evaluate_generation(model, batches_of(real, tl, 16), source="generate", key=4, k=3, mixture=None)
    # (re-batched: identical integers; the Frechet distance to the rounding the encoder's own batch dependence leaves, 1e-6 of it)
    assert all(a[q] == b[q] for q in ("precision", "recall", "density", "coverage", "n")) and abs(a["frechet"] - b["frechet"]) <= 1e-6 * a["frechet"]
    assert old == old2 and a["n"] == KR.EVAL_TEST and a["frechet"] != old["frechet"] and math.isfinite(a["frechet"])
    with pytest.raises(ValueError, match="mixture"):
        S.evaluate_generation(model, batches_of(real, tl, 16), source="mixture", key=4)
    with pytest.raises(ValueError, match="mixture"):
        S.evaluate_generation(model, batches_of(real, tl, 16), source="generate", mixture=gm, key=4)
    # evaluate_detection: the score is score_samples of the posterior means
    out = [torch.flip(ti, dims=(2,)) * 0.5]
    det = S.evaluate_detection(model, batches_of(ti, tl, 16), out, score="mixture", mixture=gm)
    values = torch.cat([gm.score_samples(S.encode_posterior(model, x)[0]) for x in (ti, out[0])])
    positive = torch.cat([torch.ones(ti.shape[0], dtype=torch.int64), torch.zeros(out[0].shape[0], dtype=torch.int64)]).to(dev())
    want = S.detection_metrics(values, positive)
    assert type(det) is type(want) and all(torch.equal(a, b) for a, b in zip(det, want))
    msp = S.evaluate_detection(model, batches_of(ti, tl, 16), out)
    msp2 = S.evaluate_detection(model, batches_of(ti, tl, 12), out, score="msp", mixture=None)
    assert all(torch.equal(a, b) for a, b in zip(msp, msp2))
    with pytest.raises(ValueError, match="mixture"):
        S.evaluate_detection(model, [ti], out, score="mixture")
    with pytest.raises(ValueError, match="mixture"):
        S.evaluate_detection(model, [ti], out, score="msp", mixture=gm)
