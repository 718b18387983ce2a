"""Latent-space clustering on a real MI355X: sv_kmeans_assign, sv_kmeans_accum, sv_kmeans_finish and sv_contingency through the C ABI
against the float64 restatement of tests/_cluster_ref.py (pinned to scikit-learn / scipy / brute force by tests/test_cluster_cpu.py),
then the Python layer (shot_vae_amd.cluster: kmeans_plus_plus, KMeans, evaluate_clustering).

Integer-valued inputs are compared exactly (fp32 and double are exact on them).  Otherwise the allowances follow the project's 8x rule
and are measured when the test runs, never taken from a GPU result: 8 x the error of the fp32 numpy restatement against float64 on the
case's own inputs (R.allowance for a pair value; shift32 / the fp32 sums below for `stats`).  An assignment is compared with float64
only on the rows whose float64 margin between the best and the second-best centroid exceeds twice the pair allowance; the inputs are
separated blobs, and the share of rows left out is asserted (on the CPU side) to stay under 1 %.  Outputs are pre-filled and carry
guard rows.

Measured on an MI355X, error (allowance): sv_kmeans_assign's dist against float64 on the blobs 8.3e-8 (4.6e-3) at (65, 2, 15), 4.2e-7
(0.16) at (130, 10, 128), 1.4e-7 (4.3) at (130, 65, 17), 6.0e-7 (0.24) at (4097, 10, 130), no row undecided in any case; stats[0] 1.6e-5
.. 1.8e-4 (1.3e-4 .. 1.4e-3) and stats[1] 2.6e-5 .. 1.9e-3 (2.0e-3 .. 3.1e-2) over the four random cases -- both are the rounding of
the fp32 result itself, an eighth of the allowance; the other comparisons are equalities or 1-ulp bounds."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import shot_vae_amd as S                                        # noqa: E402
from shot_vae_amd import _lib as L                              # noqa: E402
from oracle import closed_form as CF                            # noqa: E402
from tests import _cluster_ref as R                             # noqa: E402
from tests import _knn_ref as KR                                # noqa: E402

GUARD = 3
EUCLID = 2                                                      # SV_DIST_EUCLID


def dev():
    return torch.device("cuda:0")


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev())


def i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev())


def integers(shape, stream, lo=-2.0, hi=3.0):
    return np.floor(CF.uniform(shape, stream, lo, hi).numpy().astype(np.float64))


def ulp32(a):
    return np.spacing(np.abs(np.asarray(a, dtype=np.float32))).astype(np.float64)


# ================================================================================================ sv_kmeans_assign
def assign(x, c, cuts=None, want_dist=True):
    """sv_kmeans_assign over the rows cut at `cuts` -> (assign int64 numpy [N], dist fp32 numpy [N]); the guard rows stay as they were"""
    N, D = x.shape
    dx, dc = f32(x), f32(c)
    a = torch.full((N + GUARD,), -7, dtype=torch.int64, device=dev())
    v = torch.full((N + GUARD,), -7.0, dtype=torch.float32, device=dev())
    edges = [0] + list(cuts or []) + [N]
    for lo, hi in zip(edges[:-1], edges[1:]):
        L.call("sv_kmeans_assign", p(dx[lo:]), hi - lo, p(dc), c.shape[0], D, p(a[lo:]), p(v[lo:]) if want_dist else None, st())
    torch.cuda.synchronize()
    assert bool((a[N:] == -7).all()) and bool((v[N:] == -7.0).all()), "sv_kmeans_assign wrote behind its outputs"
    if not want_dist:
        assert bool((v == -7.0).all())
    return a[:N].cpu().numpy(), v[:N].cpu().numpy()


def pairdist(x, c):
    out = torch.full((x.shape[0], c.shape[0]), float("nan"), dtype=torch.float32, device=dev())
    dx, dc = f32(x), f32(c)
    L.call("sv_pairdist", EUCLID, p(dx), None, x.shape[0], p(dc), None, c.shape[0], x.shape[1], p(out), c.shape[0], st())
    torch.cuda.synchronize()
    return out.cpu().numpy()


ASSIGN_SHAPES = [(1, 1, 1), (63, 2, 15), (65, 10, 16), (130, 65, 17), (64, 257, 128), (130, 1024, 130)]      # N, K, D


@pytest.mark.parametrize("N,K,D", ASSIGN_SHAPES)
def test_assign_is_the_first_minimum_of_sv_pairdist_bit_for_bit(N, K, D):
    x, c = KR.posterior(N, D, 7101)[0], KR.posterior(K, D, 7103)[0]
    m = pairdist(x, c)
    want_a, want_v = R.assign(None, None, dist=m)
    a, v = assign(x, c)
    assert np.array_equal(a, want_a) and np.array_equal(v, want_v.astype(np.float32))
    assert np.array_equal(assign(x, c, want_dist=False)[0], want_a)


@pytest.mark.parametrize("N,K,D", [(130, 10, 128), (65, 2, 15), (130, 65, 17), (4097, 10, 130)])
def test_assign_matches_float64_on_the_decided_rows(N, K, D):
    x, c, _ = R.blobs(N, K, D, 7105)
    c = (c + 0.125).astype(np.float32).astype(np.float64)          # centroids beside the centres
    ref_a, ref_v = R.assign(x, c)
    tol = R.allowance(x, c)
    decided = R.margin(x, c) > 2.0 * tol
    assert (~decided).sum() <= N // 100, "the reference alone leaves more than 1 % of the rows undecided"
    a, v = assign(x, c)
    err = float(np.abs(v.astype(np.float64) - ref_v).max())
    print("FIG assign %s err %.3e tol %.3e undecided %d" % ((N, K, D), err, tol, int((~decided).sum())))
    assert np.array_equal(a[decided], ref_a[decided]) and err <= tol
    assert (a >= 0).all() and (a < K).all()


@pytest.mark.parametrize("N,K,D", [(130, 65, 1), (65, 10, 17), (63, 257, 16)])
def test_assign_breaks_exact_ties_by_the_smaller_index(N, K, D):
    x, c = integers((N, D), 7107, 0.0, 2.0), integers((K, D), 7108, 0.0, 2.0)          # binary rows: Hamming distances, ties abound
    ref_a, ref_v = R.assign(x, c)
    d = R.distances(x, c)
    assert ((d == d.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum() >= N // 4, "the case has no ties"
    for cuts in (None, [1, 64] if N > 64 else [1], [N // 2]):
        a, v = assign(x, c, cuts=cuts)
        assert np.array_equal(a, ref_a) and np.array_equal(v.astype(np.float64), ref_v)


def test_assign_gives_minus_one_where_no_value_is_finite():
    N, K, D = 70, 66, 17
    x, c = KR.posterior(N, D, 7109)[0], KR.posterior(K, D, 7111)[0]
    x[3, 5] = np.nan
    x[65, 0] = np.inf
    x[66, 16] = -np.inf
    c[0, 2] = np.nan                                       # a NaN centroid is never the minimum
    c[65, 1] = np.inf
    a, v = assign(x, c)
    bad = np.array([3, 65, 66])
    good = np.setdiff1d(np.arange(N), bad)
    assert (a[bad] == -1).all() and np.isposinf(v[bad]).all()
    ref_a, ref_v = R.assign(x[good], c[1:65])
    tol = R.allowance(x[good], c[1:65])
    decided = R.margin(x[good], c[1:65]) > 2.0 * tol
    assert np.array_equal(a[good][decided], ref_a[decided] + 1) and np.isfinite(v[good]).all()
    assert np.abs(v[good] - ref_v).max() <= tol
    a, v = assign(x, np.full((K, D), np.nan))              # every centroid NaN
    assert (a == -1).all() and np.isposinf(v).all()


def test_assign_does_not_depend_on_how_the_rows_are_cut():
    N, K, D = 1000, 65, 130
    x, c = KR.posterior(N, D, 7113)[0], KR.posterior(K, D, 7115)[0]
    one = assign(x, c)
    for cuts in ([1, 257], list(range(100, 1000, 100))):
        got = assign(x, c, cuts=cuts)
        assert np.array_equal(one[0], got[0]) and np.array_equal(one[1], got[1]), cuts


# ================================================================================================ sv_kmeans_accum / sv_kmeans_finish
def accum(x, a, v, K, P, cuts=None, fill=7.0):
    """sv_kmeans_accum over the rows cut at `cuts` (the first call has init = 1 and finds garbage in the states) -> device tensors
    (sums [P, K, D], counts [P, K], inertia [P]); the guard space behind the states stays as it was"""
    N, D = x.shape
    dx, da, dv = f32(x), i64(a), f32(v)
    sums = torch.full((P * K * D + GUARD,), fill, dtype=torch.float64, device=dev())
    counts = torch.full((P * K + GUARD,), -7, dtype=torch.int64, device=dev())
    inertia = torch.full((P + GUARD,), fill, dtype=torch.float64, device=dev())
    edges = [0] + list(cuts or []) + [N]
    for n, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
        L.call("sv_kmeans_accum", p(dx[lo:]), p(da[lo:]), p(dv[lo:]), hi - lo, D, K, p(sums), p(counts), p(inertia), P, 1 if n == 0 else 0, st())
    torch.cuda.synchronize()
    assert bool((sums[P * K * D:] == fill).all()) and bool((counts[P * K:] == -7).all()) and bool((inertia[P:] == fill).all()), \
        "sv_kmeans_accum wrote behind its states"
    return sums[:P * K * D].view(P, K, D), counts[:P * K].view(P, K), inertia[:P]


def finish(sums, counts, inertia, c_old, alias=False):
    """-> numpy (c_new fp32 [K, D], count int64 [K], stats fp32 [2])"""
    P, K, D = sums.shape
    old = f32(c_old)
    new = old if alias else torch.full((K * D + GUARD,), -7.0, dtype=torch.float32, device=dev())
    count = torch.full((K + GUARD,), -7, dtype=torch.int64, device=dev())
    stats = torch.full((2 + GUARD,), -7.0, dtype=torch.float32, device=dev())
    L.call("sv_kmeans_finish", p(sums), p(counts), p(inertia), P, K, D, p(old), p(new), p(count), p(stats), st())
    torch.cuda.synchronize()
    assert bool((count[K:] == -7).all()) and bool((stats[2:] == -7.0).all()) and (alias or bool((new[K * D:] == -7.0).all())), \
        "sv_kmeans_finish wrote behind its outputs"
    assert alias or torch.equal(old, f32(c_old)), "sv_kmeans_finish changed c_old"
    return new[:K * D].view(K, D).cpu().numpy(), count[:K].cpu().numpy(), stats[:2].cpu().numpy()


def merged(sums, counts, inertia):
    """the P states added in index order, as sv_kmeans_finish adds them"""
    s, n, i = sums[0].clone(), counts[0].clone(), inertia[0].clone()
    for q in range(1, sums.shape[0]):
        s, n, i = s + sums[q], n + counts[q], i + inertia[q]
    return s.cpu().numpy(), n.cpu().numpy(), float(i)


def labels_for(N, K, stream, holes=True):
    """an assignment with every cluster but K - 1 used, and (holes) rows outside [0, K): -1, K and a large value"""
    a = (np.floor(CF.uniform((N,), stream, 0.0, 1.0).numpy().astype(np.float64) * max(K - 1, 1))).astype(np.int64)
    if holes and N > 8:
        a[1], a[N // 2], a[N - 2] = -1, K, 2 ** 40
    return a


@pytest.mark.parametrize("N,K,D,P", [(1, 1, 1, 1), (63, 2, 15, 1), (65, 10, 16, 2), (130, 64, 17, 3), (193, 65, 128, 3), (130, 257, 130, 2),
                                     (257, 1024, 17, 4)])
def test_accum_and_finish_are_exact_on_integer_data(N, K, D, P):
    x = integers((N, D), 7201, -8.0, 9.0)
    a = labels_for(N, K, 7203)
    v = integers((N,), 7205, 0.0, 50.0)
    c_old = integers((K, D), 7207)
    sums, counts, inertia = accum(x, a, v, K, P)
    ref_c, ref_n, ref_s, ref_i = R.update(x, a, c_old, v)
    s, n, i = merged(sums, counts, inertia)
    assert np.array_equal(s, ref_s) and np.array_equal(n, ref_n) and i == ref_i
    # tile t went to state t mod P
    for q in range(P):
        rows = np.nonzero((np.arange(N) // 64) % P == q)[0]
        part = R.update(x[rows], a[rows], c_old, v[rows])
        assert np.array_equal(sums[q].cpu().numpy(), part[2]) and np.array_equal(counts[q].cpu().numpy(), part[1])
        assert float(inertia[q]) == part[3]
    c_new, count, stats = finish(sums, counts, inertia, c_old)
    assert np.array_equal(count, ref_n) and np.array_equal(c_new, ref_c.astype(np.float32))
    if K > 1:
        assert count[K - 1] == 0 and np.array_equal(c_new[K - 1], c_old[K - 1].astype(np.float32)), "an empty cluster keeps its centroid"
    want = np.float32(R.shift(ref_c.astype(np.float32), c_old))
    assert abs(float(stats[0]) - float(want)) <= float(np.spacing(want)) and stats[1] == np.float32(ref_i)
    # c_new may alias c_old
    c_alias, count2, stats2 = finish(sums, counts, inertia, c_old, alias=True)
    assert np.array_equal(c_alias, c_new) and np.array_equal(count2, count) and np.array_equal(stats2, stats)


def shift32(x, a, c_old):
    """the fp32 restatement of stats[0]: sums, centroids and the shift in fp32, index order"""
    K = c_old.shape[0]
    ok = (a >= 0) & (a < K)
    s = np.zeros(c_old.shape, dtype=np.float32)
    np.add.at(s, a[ok], x[ok].astype(np.float32))
    n = np.bincount(a[ok], minlength=K)
    c = np.where(n[:, None] > 0, s / np.maximum(n, 1)[:, None].astype(np.float32), c_old.astype(np.float32)).astype(np.float32)
    d = c - c_old.astype(np.float32)
    return float(np.sum(d * d, dtype=np.float32))


@pytest.mark.parametrize("N,K,D,P", [(130, 10, 128, 2), (193, 65, 17, 3), (257, 257, 15, 1), (4097, 1024, 16, 64)])
def test_accum_and_finish_match_float64_on_random_data(N, K, D, P):
    x = KR.posterior(N, D, 7209)[0]
    c_old = KR.posterior(K, D, 7211)[0]
    a = labels_for(N, K, 7213)
    v = (np.abs(KR.posterior(N, 1, 7215)[0][:, 0]) * D).astype(np.float32).astype(np.float64)
    sums, counts, inertia = accum(x, a, v, K, P)
    c_new, count, stats = finish(sums, counts, inertia, c_old)
    ref_c, ref_n, _, ref_i = R.update(x, a, c_old, v)
    assert np.array_equal(count, ref_n)
    near = ref_c.astype(np.float32)
    assert (np.abs(c_new.astype(np.float64) - near.astype(np.float64)) <= ulp32(near)).all(), "a centroid is more than 1 ulp from float64's"
    ref_shift = R.shift(ref_c, c_old)
    tol0 = 8.0 * abs(shift32(x, a, c_old) - ref_shift)
    ok = (a >= 0) & (a < K)
    tol1 = 8.0 * abs(float(np.sum(v[ok].astype(np.float32), dtype=np.float32)) - ref_i)
    tol1 = max(tol1, 8.0 * float(np.spacing(np.float32(ref_i))))          # (never below the rounding of the fp32 result itself)
    print("FIG stats %s shift err %.3e tol %.3e inertia err %.3e tol %.3e" % ((N, K, D, P), abs(float(stats[0]) - ref_shift), tol0,
                                                                         abs(float(stats[1]) - ref_i), tol1))
    assert abs(float(stats[0]) - ref_shift) <= tol0 and abs(float(stats[1]) - ref_i) <= tol1
    # a repeated call sequence gives the same bits
    again = accum(x, a, v, K, P, fill=-3.0)
    assert all(torch.equal(u, w) for u, w in zip((sums, counts, inertia), again))
    c2, n2, s2 = finish(*again, c_old)
    assert np.array_equal(c2, c_new) and np.array_equal(n2, count) and np.array_equal(s2, stats)


@pytest.mark.parametrize("N,K,D,P,cuts", [(449, 10, 17, 1, [64]), (449, 10, 17, 1, [128, 192, 448]), (64 * 3 * 3 + 1, 65, 16, 3, [192]),
                                          (64 * 3 * 3 + 1, 65, 16, 3, [192, 576]), (64 * 64 + 1, 257, 15, 64, [4096])])
def test_accum_cut_into_calls_gives_the_bits_of_one_call(N, K, D, P, cuts):
    """P = 1: any cut at a multiple of 64; P > 1: at a multiple of 64 P"""
    assert all(c % (64 * P) == 0 for c in cuts)
    x = KR.posterior(N, D, 7217)[0]
    a = labels_for(N, K, 7219)
    v = np.abs(KR.posterior(N, 1, 7221)[0][:, 0])
    one = accum(x, a, v, K, P)
    got = accum(x, a, v, K, P, cuts=cuts)
    assert all(torch.equal(u, w) for u, w in zip(one, got))


def test_accum_p64_on_64_tiles_and_without_inertia():
    N, K, D, P = 64 * 64, 10, 17, 64
    x = integers((N, D), 7223, -8.0, 9.0)
    a = labels_for(N, K, 7225)
    v = integers((N,), 7227, 0.0, 50.0)
    sums, counts, inertia = accum(x, a, v, K, P)
    for q in (0, 31, 63):                                  # one tile per state
        rows = np.arange(64 * q, 64 * q + 64)
        part = R.update(x[rows], a[rows], np.zeros((K, D)), v[rows])
        assert np.array_equal(sums[q].cpu().numpy(), part[2]) and np.array_equal(counts[q].cpu().numpy(), part[1])
        assert float(inertia[q]) == part[3]
    # dist and inertia may both be NULL: sums and counts alone, stats[1] = 0
    dx, da = f32(x), i64(a)
    s2, n2 = torch.empty_like(sums), torch.empty_like(counts)
    L.call("sv_kmeans_accum", p(dx), p(da), None, N, D, K, p(s2), p(n2), None, P, 1, st())
    c_old = f32(np.zeros((K, D)))
    c_new, count, stats = torch.empty_like(c_old), torch.empty(K, dtype=torch.int64, device=dev()), torch.empty(2, device=dev())
    L.call("sv_kmeans_finish", p(s2), p(n2), None, P, K, D, p(c_old), p(c_new), p(count), p(stats), st())
    torch.cuda.synchronize()
    assert torch.equal(s2, sums) and torch.equal(n2, counts) and float(stats[1]) == 0.0
    assert np.array_equal(count.cpu().numpy(), R.update(x, a, np.zeros((K, D)))[1])


# ================================================================================================ sv_contingency
def table(a, b, Ka, Kb, calls=1, into=None):
    t, counts = into if into is not None else (torch.zeros(Ka * Kb + GUARD, dtype=torch.int64, device=dev()),
                                               torch.zeros(2 + GUARD, dtype=torch.int64, device=dev()))
    da, db = i64(a), i64(b)
    for _ in range(calls):
        L.call("sv_contingency", p(da), p(db), len(a), Ka, Kb, p(t), p(counts), st())
    torch.cuda.synchronize()
    assert bool((t[Ka * Kb:] == 0).all()) and bool((counts[2:] == 0).all()), "sv_contingency wrote behind its outputs"
    return t, counts


def draw_labels(N, K, stream, lo=-1):
    """uniform over [lo, K]: both ends are outside [0, K) when lo = -1"""
    return np.floor(CF.uniform((N,), stream, float(lo), float(K + 1)).numpy().astype(np.float64)).astype(np.int64)


@pytest.mark.parametrize("N,Ka,Kb", [(1, 1, 1), (1, 3, 4), (130, 2, 2), (5000, 10, 10), (2049, 3, 257), (5000, 1024, 1024), (4097, 1, 2 ** 20)])
def test_contingency_is_exact(N, Ka, Kb):
    a, b = draw_labels(N, Ka, 7301), draw_labels(N, Kb, 7303)
    if N > 4:
        a[0], b[1], a[2], b[2] = 2 ** 40, -2 ** 40, Ka, Kb          # far outside, on either side and on both
    ref_t, ref_c = R.contingency(a, b, Ka, Kb)
    t, counts = table(a, b, Ka, Kb)
    assert np.array_equal(t[:Ka * Kb].view(Ka, Kb).cpu().numpy(), ref_t) and np.array_equal(counts[:2].cpu().numpy(), ref_c)
    assert N < 100 or 0 < ref_c[0] < N
    # everything accumulates across calls
    a2, b2 = draw_labels(max(N // 2, 1), Ka, 7305, lo=0), draw_labels(max(N // 2, 1), Kb, 7307, lo=0)
    t, counts = table(a2, b2, Ka, Kb, calls=2, into=(t, counts))
    ref2_t, ref2_c = R.contingency(a2, b2, Ka, Kb)
    assert np.array_equal(t[:Ka * Kb].view(Ka, Kb).cpu().numpy(), ref_t + 2 * ref2_t)
    assert np.array_equal(counts[:2].cpu().numpy(), ref_c + 2 * ref2_c)


def test_contingency_of_one_hot_cell():
    """every row in the same cell: the block's private count, one atomic"""
    N = 5000
    t, counts = table(np.full(N, 2), np.full(N, 1), 3, 2)
    want = np.zeros((3, 2), dtype=np.int64)
    want[2, 1] = N
    assert np.array_equal(t[:6].view(3, 2).cpu().numpy(), want) and counts[:2].tolist() == [N, N]
    assert torch.equal(S.contingency(i64(np.full(N, 2)), i64(np.full(N, 1)), 3, 2), t[:6].view(3, 2))


# ================================================================================================ kmeans_plus_plus
@pytest.mark.parametrize("N,K,D", [(130, 10, 17), (65, 65, 2), (4097, 5, 16)])
def test_kmeans_plus_plus_draws_the_restatements_rows(N, K, D):
    x = integers((N, D), 7401, -6.0, 7.0)
    distinct = len(np.unique(x, axis=0))
    for seed in (0, 1):
        u = np.random.RandomState(7403 + seed).uniform(size=K)
        cen, idx = S.kmeans_plus_plus(f32(x), K, torch.from_numpy(u).to(dev()))
        idx = idx.cpu().numpy()
        assert np.array_equal(idx, R.plus_plus(x, K, u))
        assert np.array_equal(cen.cpu().numpy(), x[idx].astype(np.float32)), "a centroid is not a row of the data"
        if distinct >= K:
            assert len(np.unique(x[idx], axis=0)) == K, "two centroids coincide"
    assert distinct >= K or N == 65


def test_kmeans_plus_plus_never_draws_a_chosen_row_again():
    x = np.repeat(integers((5, 3), 7405, -6.0, 7.0), 4, axis=0)          # 5 distinct rows, 4 copies each
    assert len(np.unique(x, axis=0)) == 5
    u = np.array([0.999, 0.0, 0.999999, 0.5, 0.25])
    cen, idx = S.kmeans_plus_plus(f32(x), 5, torch.from_numpy(u).to(dev()))
    assert np.array_equal(idx.cpu().numpy(), R.plus_plus(x, 5, u)) and len(np.unique(cen.cpu().numpy(), axis=0)) == 5


# ================================================================================================ KMeans
def blob_case(N=449, K=10, D=17, stream=7501):
    """rows of K separated blobs, the blob of every row, and starting centroids 0.4 of the way from each centre to its neighbour: every
    row's nearest start is its own blob's, by a wide margin, and the first iteration moves every centroid"""
    x, cen, which = R.blobs(N, K, D, stream)
    toward = np.concatenate([cen[1:], cen[-2:-1]])              # the next centre; the last one looks back
    start = (cen + 0.4 * (toward - cen)).astype(np.float32).astype(np.float64)
    return x, which, start


def test_kmeans_iterations_follow_the_restatement():
    x, which, start = blob_case()
    N, K = len(x), len(start)
    dx = f32(x)
    km = S.KMeans(K, x.shape[1], init=f32(start)).reset()
    c = start.copy()
    for it in range(4):
        tol = R.allowance(x, c)
        assert R.margin(x, c).min() > 2.0 * tol, "the reference itself is undecided on a row"
        a, c_new, count, inertia = R.lloyd(x, c)
        got_a, got_v = km.predict(dx, return_distance=True)
        assert np.array_equal(got_a.cpu().numpy(), a)                 # no row is left out
        stats = km.step(dx)
        got_c = km.centroids.cpu().numpy()
        near = c_new.astype(np.float32)
        assert (np.abs(got_c.astype(np.float64) - near.astype(np.float64)) <= ulp32(near)).all()
        assert np.array_equal(km.counts.cpu().numpy(), count) and km.n_iter == it + 1
        # (N distances, each within the pair allowance, and the rounding of the fp32 result)
        assert abs(float(stats[1]) - inertia) <= N * tol + float(np.spacing(np.float32(inertia)))
        c = c_new
    # the blobs are found: one cluster per blob
    t = R.contingency(which, km.predict(dx).cpu().numpy(), K, K)[0]
    assert R.metrics(t)["ari"] == 1.0 and S.partition_metrics(S.contingency(i64(which), km.predict(dx), K, K))["accuracy"] == 1.0


def test_kmeans_is_exact_on_integer_rows():
    x = integers((257, 16), 7503, -8.0, 9.0)
    start = x[R.plus_plus(x, 5, np.random.RandomState(7).uniform(size=5))]
    km = S.KMeans(5, 16, init=f32(start)).reset()
    a, c_new, count, inertia = R.lloyd(x, start)
    stats = km.step(f32(x))
    assert np.array_equal(km.centroids.cpu().numpy(), c_new.astype(np.float32)) and np.array_equal(km.counts.cpu().numpy(), count)
    assert float(stats[1]) == inertia


def test_kmeans_fit_without_tolerance_reads_nothing_and_step_predict_replay():
    """torch.cuda.graph refuses a capture that synchronises with the host: fit(tol=None), step and predict are captured whole and
    replayed onto new rows"""
    xs = [f32(blob_case(stream=s)[0]) for s in (7505, 7507)]
    start = f32(blob_case(stream=7505)[2])
    K, D = start.shape
    sx = xs[0].clone()
    fitted, stepper = S.KMeans(K, D, init=start), S.KMeans(K, D, init=start).reset()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                           # warm-up outside the capture
        fitted.fit(sx, max_iter=3, tol=None)
        stepper.step(sx)
        stepper.predict(sx, return_distance=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    stepper.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fitted.fit(sx, max_iter=3, tol=None)
        stats = stepper.step(sx)
        pred, dist = stepper.predict(sx, return_distance=True)
    for x in (xs[1], xs[0]):
        sx.copy_(x)
        stepper.centroids.copy_(start)
        graph.replay()
        torch.cuda.synchronize()
        eager = S.KMeans(K, D, init=start).fit(x, max_iter=3, tol=None)
        assert torch.equal(fitted.centroids, eager.centroids) and torch.equal(fitted.counts, eager.counts)
        assert torch.equal(fitted.inertia, eager.inertia) and eager.n_iter == 3
        one = S.KMeans(K, D, init=start).reset()
        want_stats = one.step(x)
        want_pred, want_dist = one.predict(x, return_distance=True)
        assert torch.equal(stats, want_stats) and torch.equal(stepper.centroids, one.centroids)
        assert torch.equal(pred, want_pred) and torch.equal(dist, want_dist)
    assert not torch.equal(S.KMeans(K, D, init=start).fit(xs[0], max_iter=3, tol=None).centroids,
                           S.KMeans(K, D, init=start).fit(xs[1], max_iter=3, tol=None).centroids)


def test_kmeans_fit_stops_by_the_tolerance_and_keeps_the_best_of_n_init():
    x, which, _ = blob_case(N=449, K=6, D=15, stream=7509)
    dx = f32(x)
    km = S.KMeans(6, 15, seed=3).fit(dx, max_iter=50, tol=1e-4)
    assert 1 <= km.n_iter < 50, "separated blobs converge in a few iterations"
    again = S.KMeans(6, 15, seed=3).fit(dx, max_iter=50, tol=1e-4)
    assert torch.equal(km.centroids, again.centroids) and torch.equal(km.inertia, again.inertia) and km.n_iter == again.n_iter
    a, v = km.predict(dx, return_distance=True)
    assert abs(float(km.inertia) - float(v.double().sum())) <= 8.0 * float(np.spacing(np.float32(float(km.inertia))))
    assert np.array_equal(km.counts.cpu().numpy(), np.bincount(a.cpu().numpy(), minlength=6))
    # n_init: the runs of one generator, replayed by hand with the public pieces; the least inertia wins
    best = S.KMeans(6, 15, init="random", seed=11).fit(dx, max_iter=2, tol=None, n_init=4)
    gen = torch.Generator().manual_seed(11)
    runs = []
    for _ in range(4):
        one = S.KMeans(6, 15, init="random", seed=11).reset(dx, generator=gen)
        one.step(dx)
        one.step(dx)
        runs.append((float(one.predict(dx, return_distance=True)[1].double().sum()), one.centroids))
    order = sorted(range(4), key=lambda r: runs[r][0])
    assert runs[order[0]][0] < runs[order[-1]][0], "the case cannot tell the runs apart"
    assert torch.equal(best.centroids, runs[order[0]][1])
    assert abs(float(best.inertia) - runs[order[0]][0]) <= 8.0 * float(np.spacing(np.float32(runs[order[0]][0])))


# ================================================================================================ evaluate_clustering
_MODELS = {}


def eval_model(kind):
    m = _MODELS.get(kind)
    if m is None:
        if kind == "svhn":
            m = S.svhn_VAE((3, 32, 32), {"cont": 32, "disc": [KR.EVAL_CLASSES]}, compute_dtype="fp32")
        else:
            m = S.VariationalAutoEncoder(kind, num_input_channels=3, img_size=(32, 32), data_parallel=False, continuous_latent_dim=128,
                                         disc_latent_dim=KR.EVAL_CLASSES, small_input=True, compute_dtype="fp32")
        m.load_state_dict(KR.eval_state(kind))
        m = _MODELS[kind] = m.cuda().eval()
    return m


@pytest.mark.parametrize("kind", KR.EVAL_KINDS)
@pytest.mark.parametrize("method,args", [("posterior", {}), ("kmeans", dict(k=4, seed=5, max_iter=5, tol=None))])
def test_evaluate_clustering_matches_the_restatement_on_its_own_clusters(kind, method, args):
    model = eval_model(kind)
    _, _, images, labels = (t.to(dev()) for t in KR.eval_images(kind))
    labels = labels.clone()
    labels[5] = -1                                          # a label outside the code: in no cell, still a row of its cluster
    batches = lambda B: [(images[i:i + B], labels[i:i + B]) for i in range(0, images.shape[0], B)]          # noqa: E731
    res = S.evaluate_clustering(model, batches(16), method=method, **args)
    k = args.get("k", KR.EVAL_CLASSES)
    cluster = res["clusters"].cpu().numpy()
    assert cluster.shape == (KR.EVAL_TEST,) and cluster.min() >= 0 and cluster.max() < k
    if method == "posterior":
        qy = torch.cat([model.encode(x)[2].detach() for x, _ in batches(16)]).double().cpu().numpy()
        assert np.array_equal(cluster, np.argmax(qy, axis=1)), "not the first maximum of the discrete posterior"
    ref_t = R.contingency(labels.cpu().numpy(), cluster, KR.EVAL_CLASSES, k)[0]
    ref = R.metrics(ref_t)
    assert res["n"] == ref["n"] == KR.EVAL_TEST - 1
    for name in ("accuracy", "purity", "nmi", "ari", "homogeneity", "completeness", "v_measure"):
        assert abs(res[name] - ref[name]) <= 1e-12, name
    assert np.array_equal(res["counts"], np.bincount(cluster, minlength=k)) and res["mapping"].shape == (k,)
    # re-batched: identical
    other = S.evaluate_clustering(model, batches(12), method=method, **args)
    assert torch.equal(other["clusters"], res["clusters"]) and np.array_equal(other["counts"], res["counts"])
    assert all(other[name] == res[name] for name in ("accuracy", "purity", "nmi", "ari", "homogeneity", "completeness", "v_measure", "n"))
