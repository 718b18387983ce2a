"""Generation-quality metrics on a real MI355X: sv_ball_scan through the C ABI -- exact against the project's own pair values
(sv_pairdist's matrix compared in torch), bracketed by the float64 restatement of tests/_quality_ref.py, exact on integer data, the same
integers for any cut and any P, the radius / row / self / counter rules --, then the Python layer (shot_vae_amd.quality: Manifold,
manifold_metrics, FeatureMoments, frechet_distance, evaluate_generation).

Allowances are derived, never taken from a GPU result: a pair is undecided when its float64 value is within 4 x the 8x-rule tolerance
(tests/_knn_ref.tolerance_for) of its radius; a moment sum of n terms is within 8 x n x 2^-53 x sum |terms| of the two-pass float64
one; a Frechet distance within 1e-9 of tr S1 + tr S2 of the restatement's.  Counters are pre-filled and carry guard elements.

Measured on an MI355X: undecided pairs 28 (euclid) / 3 (w2) of 9 100 at D = 1, 0 in every other case; precision 0.40 .. 0.99, coverage
0.56 .. 1.0 over the cases; 28 boundary pairs per integer-data case; moments: mean error 0 .. 3.6e-15 (2.5e-12 .. 5.4e-12), covariance
6.7e-16 .. 5.8e-15 (2.5e-14 .. 7.0e-14); frechet_distance within 7.1e-14 / 1.4e-13 (1.1e-7 / 3.7e-7); evaluate_generation: every integer
0 on the closed-form images (an untrained decoder's samples lie far from them), precision 0.77 .. 0.94, recall 0.90 .. 1.0, coverage
0.90 .. 0.96 with the model's own samples as the real set, frechet within 2e-19 of the restatement (DESIGN.md 4g has the table)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import shot_vae_amd as S                                        # noqa: E402
from shot_vae_amd import _lib as L                              # noqa: E402
from shot_vae_amd import aggregate as AG                        # noqa: E402
from tests import _knn_ref as R                                 # noqa: E402
from tests import _quality_ref as QR                            # noqa: E402

GUARD = 5
CODE = {"euclid": L.DIST_EUCLID, "w2": L.DIST_W2}
METRICS = ("euclid", "w2")
SQ, SG = 4100, 4102                                             # the streams of the query and the gallery rows
U53 = 2.0 ** -53


def dev():
    return torch.device("cuda:0")


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev())


def launcher_p(nq, N):
    return AG.partials(-(-nq // 64), N)


def scan(metric, qm, ql, gm, gl, r, cuts=None, qcuts=None, P=None, self0=-1, want="qg", q_init=None, g_init=None):
    """sv_ball_scan over the gallery cut at `cuts` and the queries cut at `qcuts` (row offsets) -> (q_count, g_count) int64 numpy (None
    for a counter not in `want`: its pointer is NULL).  The counters start at q_init / g_init (zeros) and the guard elements around
    them must stay as they were."""
    nq, D = qm.shape
    N = gm.shape[0]
    two = metric == "w2"
    dq, dg, dr = f32(qm), f32(gm), f32(r)
    dql, dgl = (f32(ql), f32(gl)) if two else (None, None)
    bufs = {}
    for name, n, init in (("q", nq, q_init), ("g", N, g_init)):
        b = torch.full((n + 2 * GUARD,), -7, dtype=torch.int64, device=dev())
        b[GUARD:GUARD + n] = 0 if init is None else torch.from_numpy(np.asarray(init, dtype=np.int64)).to(dev())
        bufs[name] = b
    qedges, gedges = [0] + list(qcuts or []) + [nq], [0] + list(cuts or []) + [N]
    for qa, qb in zip(qedges[:-1], qedges[1:]):
        for a, b in zip(gedges[:-1], gedges[1:]):
            L.call("sv_ball_scan", CODE[metric], p(dq[qa:]), p(dql[qa:]) if two else None, qb - qa, p(dg[a:]), p(dgl[a:]) if two else None,
                   p(dr[a:]), b - a, D, a, self0 + qa if self0 >= 0 else -1, P or launcher_p(qb - qa, b - a),
                   p(bufs["q"][GUARD + qa:]) if "q" in want else None, p(bufs["g"][GUARD + a:]) if "g" in want else None, st())
    torch.cuda.synchronize()
    out = []
    for name, n, init in (("q", nq, q_init), ("g", N, g_init)):
        b = bufs[name]
        assert bool((b[:GUARD] == -7).all()) and bool((b[GUARD + n:] == -7).all()), "sv_ball_scan wrote beside %s_count" % name
        got = b[GUARD:GUARD + n].cpu().numpy()
        if name not in want:
            assert np.array_equal(got, np.zeros(n, np.int64) if init is None else np.asarray(init, np.int64)), "a NULL counter was written"
            got = None
        out.append(got)
    return out


def device_radii(metric, gm, gl, k):
    """the k-th-neighbour radii the way Manifold.fit takes them: LatentIndex.search leave-one-out; fp32 values as float64 numpy"""
    idx = S.LatentIndex(gm.shape[1], metric)
    idx.add(f32(gm), f32(gl) if metric == "w2" else None)
    val = idx.search(f32(gm), f32(gl) if metric == "w2" else None, k=k, exclude_self_from=0)[0]
    return val[:, k - 1].double().cpu().numpy()


def pair_counts(metric, qm, ql, gm, gl, r, self0=-1):
    """the counts taken from sv_pairdist's own matrix with <= in torch"""
    two = metric == "w2"
    d = S.pairwise_distance(f32(qm), f32(ql) if two else None, f32(gm), f32(gl) if two else None, metric)
    m = torch.isfinite(d) & (d <= f32(r)[None, :])
    if self0 >= 0:
        i = torch.arange(d.shape[0], device=dev())
        j = self0 + i
        ok = j < d.shape[1]
        m[i[ok], j[ok]] = False
    return m.sum(dim=1).cpu().numpy(), m.sum(dim=0).cpu().numpy()


def integer_rows(n, D, seed):
    """values in {-8 .. 8}, log sigma 0: every difference, square and sum is exact in fp32 (D x 16^2 < 2^24)"""
    return np.random.RandomState(seed).randint(-8, 9, size=(n, D)).astype(np.float64), np.zeros((n, D))


# ================================================================================================ sv_ball_scan: values
CASES = [(1, 1, 1, 0), (5, 2, 7, 1), (70, 63, 17, 1), (33, 65, 128, 5), (70, 130, 130, 3), (70, 130, 1, 3), (70, 130, 7, 3)]


def case(metric, Q, N, D, k):
    qm, ql = R.posterior(Q, D, SQ)
    gm, gl = R.posterior(N, D, SG)
    if k == 0:                                              # one gallery row has no neighbour: the radius is the pair's own value
        two = metric == "w2"
        r = S.pairwise_distance(f32(qm), f32(ql) if two else None, f32(gm), f32(gl) if two else None, metric).double().cpu().numpy().reshape(1)
    else:
        r = device_radii(metric, gm, gl, k)
    return qm, ql, gm, gl, r


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("Q,N,D,k", CASES)
def test_counts_equal_the_counts_of_the_pair_matrix(metric, Q, N, D, k):
    """integer equality with sv_pairdist's values, no allowance: the kernel's pair value is that value bit for bit"""
    qm, ql, gm, gl, r = case(metric, Q, N, D, k)
    for radii in ((r, 0.5 * r, np.full(N, np.inf)) if k == 0 else (r,)):
        want_q, want_g = pair_counts(metric, qm, ql, gm, gl, radii)
        got_q, got_g = scan(metric, qm, ql, gm, gl, radii)
        assert np.array_equal(got_q, want_q) and np.array_equal(got_g, want_g)
        assert got_q.sum() == got_g.sum()
    print("FIG pairs %s Q=%d N=%d D=%d k=%d inside %d of %d, precision %.3f coverage %.3f" % (
        metric, Q, N, D, k, got_q.sum(), Q * N, (got_q > 0).mean(), (got_g > 0).mean()))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("Q,N,D,k", CASES[1:])
def test_counts_lie_between_the_float64_sure_and_possible(metric, Q, N, D, k):
    qm, ql, gm, gl, r = case(metric, Q, N, D, k)
    ref = R.distances(metric, qm, ql, gm, gl)
    tol = 4.0 * R.tolerance_for(metric, D)
    undecided = np.abs(ref - r[None, :]) <= tol
    sure = (ref <= r[None, :]) & ~undecided
    got_q, got_g = scan(metric, qm, ql, gm, gl, r)
    prec, cov = float((got_q > 0).mean()), float((got_g > 0).mean())
    print("FIG f64 %s Q=%d N=%d D=%d k=%d undecided %d of %d, inside %d, precision %.3f coverage %.3f" % (
        metric, Q, N, D, k, undecided.sum(), Q * N, got_q.sum(), prec, cov))
    assert undecided.sum() <= 0.01 * Q * N, "the case does not decide enough pairs"
    for got, axis in ((got_q, 1), (got_g, 0)):
        lo, hi = sure.sum(axis=axis), sure.sum(axis=axis) + undecided.sum(axis=axis)
        assert (got >= lo).all() and (got <= hi).all()
    if (Q, N, D, k) == (70, 130, 7, 3):
        assert 0.0 < prec < 1.0


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("D", (7, 130))
def test_integer_data_is_exact_boundary_pairs_included(metric, D):
    qm, ql = integer_rows(70, D, 4110 + D)
    gm, gl = integer_rows(130, D, 4112 + D)
    qm[:20] = gm[30:50]                                     # coincident rows, and rows that share their neighbours' distances
    r = QR.radii(metric, gm, gl, 3)
    assert np.array_equal(device_radii(metric, gm, gl, 3), r)
    ref = R.distances(metric, qm, ql, gm, gl)
    assert (ref == r[None, :]).sum() > 0, "the case has no boundary pair"
    want_q, want_g = QR.counts(ref, r)
    got_q, got_g = scan(metric, qm, ql, gm, gl, r)
    print("FIG integer %s D=%d boundary pairs %d inside %d" % (metric, D, (ref == r[None, :]).sum(), want_q.sum()))
    assert np.array_equal(got_q, want_q) and np.array_equal(got_g, want_g)


# ================================================================================================ sv_ball_scan: cuts and P
@pytest.mark.parametrize("metric", METRICS)
def test_any_cut_and_any_p_give_the_same_integers(metric):
    Q, N, D = 65, 1000, 7
    qm, ql = R.posterior(Q, D, SQ)
    gm, gl = R.posterior(N, D, SG)
    r = device_radii(metric, gm, gl, 3)
    one_q, one_g = scan(metric, qm, ql, gm, gl, r)
    assert 0 < one_q.sum() < Q * N and np.array_equal(pair_counts(metric, qm, ql, gm, gl, r)[0], one_q)
    ref = scan(metric, qm, ql, gm, gl, r, self0=40)
    want = pair_counts(metric, qm, ql, gm, gl, r, self0=40)
    assert np.array_equal(ref[0], want[0]) and np.array_equal(ref[1], want[1])
    for cuts in (None, [1, 257], list(range(100, 1000, 100))):
        for qcuts in (None, [1]):
            for P in (1, 2, 7, 64):
                got = scan(metric, qm, ql, gm, gl, r, cuts=cuts, qcuts=qcuts, P=P, self0=40)
                assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (cuts, qcuts, P)
    again = scan(metric, qm, ql, gm, gl, r, self0=40)
    assert np.array_equal(again[0], ref[0]) and np.array_equal(again[1], ref[1])


def test_p64_on_64_tiles():
    Q, N, D = 65, 4096, 7
    qm, ql = R.posterior(Q, D, SQ)
    gm, gl = R.posterior(N, D, SG)
    r = device_radii("euclid", gm, gl, 3)
    a, b = scan("euclid", qm, ql, gm, gl, r, P=64), scan("euclid", qm, ql, gm, gl, r, P=1)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].sum() > 0
    want = pair_counts("euclid", qm, ql, gm, gl, r)
    assert np.array_equal(a[0], want[0]) and np.array_equal(a[1], want[1])


# ================================================================================================ sv_ball_scan: the rules
@pytest.mark.parametrize("metric", METRICS)
def test_radius_and_row_rules(metric):
    Q, N, D = 70, 130, 7
    qm, ql = integer_rows(Q, D, 4120)
    gm, gl = integer_rows(N, D, 4122)
    gm[6] = gm[5]                                           # duplicates: radius 0 holds the coincident rows only
    qm[7] = gm[5]
    r = QR.radii(metric, gm, gl, 3)
    r[0], r[1], r[2], r[5], r[6] = np.nan, np.inf, -1.0, 0.0, 0.0
    gm[10, 3], gm[11, 2] = np.nan, np.inf                   # a NaN / infinite row on either side is inside nothing, holds nothing
    qm[3, 0], qm[4, 2] = np.nan, -np.inf
    r[11] = np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        ref = R.distances(metric, qm, ql, gm, gl)
    want_q, want_g = QR.counts(ref, r)
    assert want_g[0] == 0 and want_g[2] == 0 and want_g[1] == Q - 2 and want_g[10] == 0 and want_g[11] == 0
    assert want_g[5] == want_g[6] == 1 and want_q[3] == 0 and want_q[4] == 0 and want_q[7] >= 3
    got_q, got_g = scan(metric, qm, ql, gm, gl, r)
    assert np.array_equal(got_q, want_q) and np.array_equal(got_g, want_g)
    # either counter NULL; the counters are added to, not overwritten
    only_q = scan(metric, qm, ql, gm, gl, r, want="q", g_init=np.arange(N) + 50)
    only_g = scan(metric, qm, ql, gm, gl, r, want="g", cuts=[64], q_init=np.arange(Q) + 50)
    assert np.array_equal(only_q[0], want_q) and only_q[1] is None and only_g[0] is None and np.array_equal(only_g[1], want_g)
    q0, g0 = np.arange(Q) * 3 + 1000, 2000 - np.arange(N)
    got_q, got_g = scan(metric, qm, ql, gm, gl, r, cuts=[1, 65], q_init=q0, g_init=g0)
    assert np.array_equal(got_q, want_q + q0) and np.array_equal(got_g, want_g + g0)


@pytest.mark.parametrize("metric", METRICS)
def test_self_exclusion(metric):
    """the queries ARE gallery rows 40 .. 109: with self0 = 40 every query leaves its own ball; self0 at the start of the columns, inside,
    partly and wholly beyond them, on the whole gallery and on one cut at 64 and 100 (col0 shifts the columns, not the rule)"""
    N, D = 130, 7
    gm, gl = integer_rows(N, D, 4124)
    qm, ql = gm[40:110].copy(), gl[40:110].copy()
    r = QR.radii(metric, gm, gl, 3)
    ref = R.distances(metric, qm, ql, gm, gl)
    base = QR.counts(ref, r)
    for self0 in (-1, 0, 40, 100, 500):
        want_q, want_g = QR.counts(ref, r, self0=self0)
        for cuts in (None, [64, 100]):
            got_q, got_g = scan(metric, qm, ql, gm, gl, r, cuts=cuts, self0=self0)
            assert np.array_equal(got_q, want_q) and np.array_equal(got_g, want_g), (self0, cuts)
        if self0 == 40:
            assert np.array_equal(want_q, base[0] - 1) and np.array_equal(want_g[40:110], base[1][40:110] - 1)
        if self0 in (-1, 500):
            assert np.array_equal(want_q, base[0])


# ================================================================================================ Manifold, manifold_metrics
def test_manifold_added_in_pieces_equals_added_at_once():
    N, D, k = 1500, 17, 4                                   # 1500 rows: the buffers grow once on the way (1024 -> 2048)
    gm, gl = R.posterior(N, D, SG)
    qm, ql = R.posterior(70, D, SQ)
    for metric in METRICS:
        ls = (lambda a: f32(a)) if metric == "w2" else (lambda a: None)
        one, three = S.Manifold(D, metric), S.Manifold(D, metric)
        assert one.add(f32(gm), ls(gl)) == 0 and len(one) == N
        assert [three.add(f32(gm[a:b]), ls(gl[a:b])) for a, b in ((0, 700), (700, 1200), (1200, N))] == [0, 700, 1200]
        with pytest.raises(ValueError, match="fit"):
            one.count(f32(qm), ls(ql))
        ra, rb = one.fit(k), three.fit(k)
        assert torch.equal(ra, rb) and ra.dtype == torch.float32 and tuple(ra.shape) == (N,) and one.k == k
        assert np.array_equal(ra.double().cpu().numpy(), device_radii(metric, gm, gl, k))
        ga, gb = (torch.zeros(N, dtype=torch.int64, device=dev()) for _ in range(2))
        ca, cb = one.count(f32(qm), ls(ql), gallery_count=ga), three.count(f32(qm), ls(ql), gallery_count=gb)
        assert torch.equal(ca, cb) and torch.equal(ga, gb) and ca.dtype == torch.int64 and tuple(ca.shape) == (70,)
        want = pair_counts(metric, qm, ql, gm, gl, ra.double().cpu().numpy())
        assert np.array_equal(ca.cpu().numpy(), want[0]) and np.array_equal(ga.cpu().numpy(), want[1])
        one.count(f32(qm), ls(ql), gallery_count=ga)                         # added to
        assert torch.equal(ga, 2 * gb)
        loo = one.count(one.mu[100:170], None if one.ls is None else one.ls[100:170], exclude_self_from=100)
        assert np.array_equal(loo.cpu().numpy(), pair_counts(metric, gm[100:170], gl[100:170], gm, gl, ra.double().cpu().numpy(), self0=100)[0])
        # errors: shapes are ValueErrors raised before any call into the library; a CPU tensor is refused; add() drops the radii
        for fn in (lambda: one.count(f32(qm)[:, :5], ls(ql)), lambda: one.count(f32(qm), ls(ql), gallery_count=ga[:-1]),
                   lambda: one.count(f32(qm), ls(ql), gallery_count=ga.int()), lambda: one.count(f32(qm), ls(ql), exclude_self_from=-2),
                   lambda: one.fit(N), lambda: one.fit(0)):
            with pytest.raises(ValueError):
                fn()
        with pytest.raises(L.ShotVaeHipError, match="MI355X"):
            one.count(f32(qm).cpu(), ls(ql))
        with pytest.raises(L.ShotVaeHipError, match="MI355X"):
            one.count(f32(qm), ls(ql), gallery_count=ga.cpu())
        one.add(f32(gm[:3]), ls(gl[:3]))
        with pytest.raises(ValueError, match="fit"):
            one.count(f32(qm), ls(ql))


@pytest.mark.parametrize("metric", METRICS)
def test_fit_and_metrics_equal_the_restatement_on_integer_data(metric):
    real_mu, real_ls = integer_rows(130, 7, 4130)
    fake_mu, fake_ls = integer_rows(70, 7, 4132)
    fake_mu[:15] = real_mu[20:35]
    fake_mu[40:] += 6.0                                     # a part of the fake set lies off the real one
    two = metric == "w2"
    man = S.Manifold(7, metric)
    man.add(f32(real_mu), f32(real_ls) if two else None)
    for k in (1, 3):
        assert np.array_equal(man.fit(k).double().cpu().numpy(), QR.radii(metric, real_mu, real_ls, k))
    got = S.manifold_metrics(f32(real_mu), f32(fake_mu), f32(real_ls) if two else None, f32(fake_ls) if two else None, k=3, metric=metric)
    want = QR.metrics(metric, real_mu, real_ls, fake_mu, fake_ls, 3)
    print("FIG manifold_metrics %s %s" % (metric, got))
    assert got == want
    assert 0.0 < got["precision"] < 1.0 and 0.0 < got["recall"] < 1.0 and 0.0 < got["coverage"] < 1.0 and got["density"] > 0.0


def test_count_under_graph_capture():
    N, D = 300, 128
    gm, _ = R.posterior(N, D, SG)
    man = S.Manifold(D)
    man.add(f32(gm))
    man.fit(5)
    near = gm[:70] + 0.05 * R.posterior(70, D, SQ)[0]        # every row inside the ball of the row it started from
    away = near.copy()
    away[35:] += 100.0                                      # half of them far from every ball
    qs = [f32(near), f32(away)]
    sq = qs[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                           # warm-up outside the capture
        man.count(sq)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = man.count(sq)
    for q in (qs[1], qs[0]):                                # replayed on new queries
        sq.copy_(q)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(got, man.count(q)) and int(got.sum()) > 0
    assert not torch.equal(man.count(qs[0]), man.count(qs[1]))


# ================================================================================================ FeatureMoments, frechet_distance
def feature_rows(n, D, stream, shift):
    """fp32 rows (as float64) with an anisotropic spread, `shift` away from the origin"""
    x = R.posterior(n, D, stream)[0] * (0.5 + np.arange(D) / D) + shift
    return x.astype(np.float32).astype(np.float64)


def moments_of(x, cuts):
    mom = S.FeatureMoments(x.shape[1])
    edges = [0] + cuts + [len(x)]
    for a, b in zip(edges[:-1], edges[1:]):
        mom.add(f32(x[a:b]))
    return mom


@pytest.mark.parametrize("n,D", [(200, 40), (96, 128)])
def test_feature_moments_match_the_two_pass_float64_moments(n, D):
    x = feature_rows(n, D, 4140, 30.0)
    for cuts in ([], [1], [64, 128] if n > 128 else [32, 64]):
        mom = moments_of(x, cuts)
        mean, cov = mom.mean(), mom.cov()
        assert mean.dtype == cov.dtype == torch.float64 and tuple(mean.shape) == (D,) and tuple(cov.shape) == (D, D) and mom.rows == n
        want_mean, want_cov = QR.moments(x)
        first = x[:(cuts[0] if cuts else n)].mean(axis=0)
        t1, t2 = QR.moment_terms(x, first)
        # 8 x n x 2^-53 x sum |terms|: the terms of the mean are (x - shift) / n and the shift itself; those of the covariance
        # (x - shift)(x - shift)^T / (n - 1) and the rank-one correction s1 s1^T / (n (n - 1)), |s1| <= sum |x - shift|
        tol_mean = 8.0 * n * U53 * (t1 / n + np.abs(first))
        tol_cov = 8.0 * n * U53 * (t2 + np.outer(t1, t1) / n) / (n - 1)
        e_mean, e_cov = np.abs(mean.cpu().numpy() - want_mean), np.abs(cov.cpu().numpy() - want_cov)
        print("FIG moments n=%d D=%d cuts %s mean err %.2e (%.2e) cov err %.2e (%.2e)" % (
            n, D, cuts, e_mean.max(), tol_mean.min(), e_cov.max(), tol_cov.min()))
        assert (e_mean <= tol_mean).all() and (e_cov <= tol_cov).all()


@pytest.mark.parametrize("na,nb,D", [(200, 150, 40), (96, 96, 128)])
def test_frechet_distance_matches_the_restatement(na, nb, D):
    a = feature_rows(na, D, 4142, 30.0)
    b = (1.3 * feature_rows(nb, D, 4144, 30.0) - 8.0).astype(np.float32).astype(np.float64)
    ma, mb = moments_of(a, [64]), moments_of(b, [32, 64])
    got, want = S.frechet_distance(ma, mb), QR.frechet_of_rows(a, b)
    tr = float(np.trace(QR.moments(a)[1]) + np.trace(QR.moments(b)[1]))
    print("FIG frechet na=%d nb=%d D=%d got %.12e want %.12e err %.2e allowance %.2e" % (na, nb, D, got, want, abs(got - want), 1e-9 * tr))
    assert abs(got - want) <= 1e-9 * tr and got > 0.01 * tr
    assert abs(S.frechet_distance(mb, ma) - got) <= 1e-9 * tr
    assert abs(S.frechet_distance(ma, moments_of(a, []))) <= 1e-9 * tr


# ================================================================================================ evaluate_generation
_MODELS = {}
EVAL_N = 96
EVAL_K, EVAL_KEY, EVAL_TAU = 5, 77, 0.9


def eval_model(kind):
    m = _MODELS.get(kind)
    if m is None:
        if kind == "svhn":
            m = S.svhn_VAE((3, 32, 32), {"cont": 32, "disc": [R.EVAL_CLASSES]}, compute_dtype="fp32")
        else:
            m = S.VariationalAutoEncoder(kind, num_input_channels=3, img_size=(32, 32), data_parallel=False, continuous_latent_dim=128,
                                         disc_latent_dim=R.EVAL_CLASSES, small_input=True, compute_dtype="fp32")
        m.load_state_dict(R.eval_state(kind))
        m = _MODELS[kind] = m.cuda().eval()
    return m


def own_rows(model, space, metric, source, x, y, b):
    """the two row sets evaluate_generation compares, made here with the model's public calls in batches of b"""
    real, fake = [], []
    for i in range(0, EVAL_N, b):
        xb = x[i:i + b]
        made = model.reconstruct(xb) if source == "reconstruct" else model.generate(y[i:i + b], EVAL_KEY, tau=EVAL_TAU, row0=i)
        for images, rows in ((xb, real), (made, fake)):
            if space == "features":
                rows.append((model.features(images).float().contiguous(), None))
            else:
                mu, ls = S.encode_posterior(model, images)
                rows.append((mu, ls if metric == "w2" else None))
    cat = lambda rows, j: None if rows[0][j] is None else torch.cat([r[j] for r in rows])          # noqa: E731
    return cat(real, 0), cat(real, 1), cat(fake, 0), cat(fake, 1)


def torch_metrics(metric, r_mu, r_ls, f_mu, f_ls, k):
    """the integer quantities from pairwise_distance + LatentIndex.search + torch compares"""
    def radii(mu, ls):
        idx = S.LatentIndex(mu.shape[1], metric)
        idx.add(mu, ls)
        return idx.search(mu, ls, k=k, exclude_self_from=0)[0][:, k - 1]
    d = S.pairwise_distance(f_mu, f_ls, r_mu, r_ls, metric)
    in_real = torch.isfinite(d) & (d <= radii(r_mu, r_ls)[None, :])
    d = S.pairwise_distance(r_mu, r_ls, f_mu, f_ls, metric)
    in_fake = torch.isfinite(d) & (d <= radii(f_mu, f_ls)[None, :])
    n_real, n_fake = r_mu.shape[0], f_mu.shape[0]
    return dict(precision=int(in_real.any(dim=1).sum()) / n_fake, recall=int(in_fake.any(dim=1).sum()) / n_real,
                density=int(in_real.sum()) / (k * n_fake), coverage=int(in_real.any(dim=0).sum()) / n_real)


@pytest.mark.parametrize("kind,source,space,metric", [
    ("wideresnet-10-1", "generate", "mu", "euclid"), ("wideresnet-10-1", "generate", "features", "euclid"),
    ("wideresnet-10-1", "reconstruct", "mu", "euclid"), ("wideresnet-10-1", "reconstruct", "features", "euclid"),
    ("svhn", "generate", "mu", "euclid"), ("svhn", "reconstruct", "mu", "euclid"), ("svhn", "generate", "mu", "w2")])
def test_evaluate_generation_matches_its_own_rows(kind, source, space, metric):
    """twice: on the closed-form images -- an untrained decoder's samples lie far from them: every integer is 0 --, and with the
    model's own samples under another key as the `real` set -- two draws of one distribution: every measure strictly inside (0, 1]"""
    model = eval_model(kind)
    images, y = (t.to(dev()) for t in R.eval_images(kind)[:2])
    assert images.shape[0] == EVAL_N
    for data, x in (("images", images), ("samples", model.generate(y, EVAL_KEY + 1, tau=EVAL_TAU, row0=0))):
        res = check_evaluate_generation(model, kind, data, x, y, source, space, metric)
        if data == "samples" and source == "generate":
            assert res["precision"] > 0.0 and res["recall"] > 0.0 and res["coverage"] > 0.0 and res["density"] > 0.0


def check_evaluate_generation(model, kind, data, x, y, source, space, metric):
    batches = lambda b: [(x[i:i + b], y[i:i + b]) for i in range(0, EVAL_N, b)]          # noqa: E731
    kw = dict(source=source, space=space, k=EVAL_K, metric=metric, key=EVAL_KEY, tau=EVAL_TAU)
    res = S.evaluate_generation(model, batches(16), **kw)
    assert set(res) == {"frechet", "precision", "recall", "density", "coverage", "n"} and res["n"] == EVAL_N
    r_mu, r_ls, f_mu, f_ls = own_rows(model, space, metric, source, x, y, 16)
    want = torch_metrics(metric, r_mu, r_ls, f_mu, f_ls, EVAL_K)
    ref = QR.frechet_of_rows(r_mu.double().cpu().numpy(), f_mu.double().cpu().numpy())
    tr = float(np.trace(QR.moments(r_mu.double().cpu().numpy())[1]) + np.trace(QR.moments(f_mu.double().cpu().numpy())[1]))
    print("FIG evaluate_generation %s %s %s %s D=%d precision %.4f recall %.4f density %.4f coverage %.4f frechet %.9e (restatement %.9e, "
          "err %.2e, allowance %.2e)" % (kind + "/" + data, source, space, metric, r_mu.shape[1], res["precision"], res["recall"], res["density"],
                                         res["coverage"], res["frechet"], ref, abs(res["frechet"] - ref), 1e-9 * tr))
    for name, v in want.items():
        assert res[name] == v, name
    assert abs(res["frechet"] - ref) <= 1e-9 * tr
    # re-batched: 96 = 6 x 16 = 2 x 48, identical integers
    again = S.evaluate_generation(model, batches(48), **kw)
    for name in want:
        assert again[name] == res[name], name
    assert abs(again["frechet"] - res["frechet"]) <= 2e-9 * tr
    if source == "generate":                                # without labels: the predicted class, on the device
        pred = torch.cat([model.predict(xb) for xb, _ in batches(16)])
        a = S.evaluate_generation(model, [(xb,) for xb, _ in batches(16)], **kw)
        b = S.evaluate_generation(model, [(xb, pred[i * 16:(i + 1) * 16]) for i, (xb, _) in enumerate(batches(16))], **kw)
        for name in want:
            assert a[name] == b[name], name
        assert abs(a["frechet"] - b["frechet"]) <= 2e-9 * tr
    return res
