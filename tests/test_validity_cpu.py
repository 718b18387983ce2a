"""Internal cluster validity without a GPU: the float64 restatement of tests/_validity_ref.py pinned to scikit-learn (the silhouette on
scipy's distance matrix, Calinski-Harabasz, Davies-Bouldin), its identities, the package's host formulas against it, the argument
refusals of sv_sil_scan / sv_sil_finish / sv_cluster_spread (they validate before any HIP call) and of shot_vae_amd.validity, and the
inputs of the GPU tests checked against their own conditions."""
import ctypes as C

import numpy as np
import pytest
import torch

import shot_vae_amd as S
from shot_vae_amd import _lib as L
from shot_vae_amd import validity as V
from tests import _validity_ref as R

SV_E_ARG = -1


# ================================================================================================ against scikit-learn
@pytest.mark.parametrize("N,K,D", R.SHAPES_CPU)
def test_the_restatement_is_scikit_learns(N, K, D):
    M = pytest.importorskip("sklearn.metrics")
    cdist = pytest.importorskip("scipy.spatial.distance").cdist
    x, lab = R.case(N, K, D, empty=False)
    sizes = np.bincount(lab, minlength=K)
    assert (sizes == 1).any() and (R.distances(R.EUCLID, x, x) + np.eye(N) == 0.0).any(), "a singleton and a pair of duplicates"
    # the silhouette on scipy's matrix (scikit-learn's own Euclid path expands the square: up to 6e-9 off on duplicates)
    want = M.silhouette_samples(cdist(x, x), lab, metric="precomputed")
    got = R.silhouette_samples(x, lab, K)
    assert np.abs(got - want).max() <= 1e-12
    want2 = M.silhouette_samples(cdist(x, x, "sqeuclidean"), lab, metric="precomputed")
    assert np.abs(R.silhouette_samples(x, lab, K, R.SQEUCLID) - want2).max() <= 1e-12
    ch, ch_want = R.calinski_harabasz(x, lab, K), M.calinski_harabasz_score(x, lab)
    assert abs(ch - ch_want) <= 1e-12 * abs(ch_want)
    db, db_want = R.davies_bouldin(x, lab, K), M.davies_bouldin_score(x, lab)
    print("FIG validity N=%d K=%d D=%d: davies_bouldin %.12e against scikit-learn's %.12e, rel %.2e" % (
        N, K, D, db, db_want, abs(db - db_want) / abs(db_want)))
    assert abs(db - db_want) <= 1e-8 * abs(db_want)


# ================================================================================================ identities
def test_identities_of_the_silhouette():
    x, lab = R.case(130, 5, 7, seed=3)
    s = R.silhouette_samples(x, lab, 5)
    assert np.isfinite(s).all() and (s >= -1.0).all() and (s <= 1.0).all()
    # renaming the clusters changes nothing (the minimum over the others is over the same set)
    perm = np.array([3, 0, 4, 1, 2])
    assert np.array_equal(R.silhouette_samples(x, perm[lab], 5), s)
    # a singleton gives 0, and K = N gives all 0
    assert s[lab == 0].tolist() == [0.0]
    assert not R.silhouette_samples(x[:20], np.arange(20), 20).any()
    # two distant blobs
    rs = np.random.RandomState(5)
    blobs = np.concatenate([rs.randn(40, 4), rs.randn(40, 4) + 30.0])
    assert R.silhouette_samples(blobs, np.repeat([0, 1], 40), 2).mean() > 0.9
    # what belongs to no cluster is NaN and in no other row's sums
    lab2 = lab.copy()
    lab2[[4, 9]] = [-1, 5]
    x2 = x.copy()
    x2[11, 2] = np.nan
    s2 = R.silhouette_samples(x2, lab2, 5)
    keep = np.ones(130, dtype=bool)
    keep[[4, 9, 11]] = False
    assert np.isnan(s2[~keep]).all() and np.array_equal(s2[keep], R.silhouette_samples(x[keep], lab[keep], 5))
    # one non-empty cluster: no value
    assert np.isnan(R.silhouette_samples(x, np.zeros(130, dtype=np.int64), 3)).all()


def test_queries_are_rows_of_the_full_result():
    """queries = n is the full result, permuted; a subset is a subset (a query's value does not depend on the other queries)"""
    x, lab = R.case(70, 4, 5, seed=4)
    g, key, order, seg = R.grouped(x, lab, 4)
    full = R.silhouette_samples(x, lab, 4)
    for m in (70, 13):
        idx = V.query_indices(70, m, 7).numpy()
        assert len(set(idx.tolist())) == m
        got = R.dense(R.distances(R.EUCLID, x[idx], g), lab[idx], seg, 4)[0]
        assert np.array_equal(got, full[idx])
    assert np.array_equal(V.query_indices(70, 13, 7).numpy(), V.query_indices(70, 70, 7).numpy()[:13])


def test_the_kernel_order_restatement_agrees_with_the_dense_one():
    x, lab = R.case(193, 65, 17)
    g, key, order, seg = R.grouped(x, lab, 65)
    for metric in (R.EUCLID, R.SQEUCLID):
        V32 = R.distances(metric, g, g, fp32=True)
        want = R.dense(V32, key, seg, 65)
        for P in (1, 3, 64):
            got = R.finish_rows(*R.ordered_parts(metric, g, key, g, seg, 65, P, V=V32), key, seg, 65, len(g))
            for a, b in zip(got, want):
                fin = np.isfinite(b)
                assert np.array_equal(np.isnan(a), np.isnan(b)) and np.abs(a[fin] - b[fin]).max() <= 1e-12 * max(1.0, np.abs(b[fin]).max())
    sums, cnts, skipped = R.cluster_sums(want[0], key, 65)
    assert skipped == int(np.isnan(want[0]).sum()) == 0 and cnts.sum() == 193
    assert abs(sums.sum() - want[0].sum()) <= 1e-12


# ================================================================================================ the package's host formulas
@pytest.mark.parametrize("N,K,D", R.SHAPES_CPU)
def test_host_formulas_against_the_restatement(N, K, D):
    x, lab = R.case(N, K, D)                                    # with an empty cluster where K >= 3: ignored
    cent, cnt, within, mean_dist = R.spread_of(x, lab, K)
    ch, db = R.calinski_harabasz(x, lab, K), R.davies_bouldin(x, lab, K)
    assert abs(V.calinski_harabasz(cent, cnt, within) - ch) <= 1e-12 * ch
    assert abs(V.davies_bouldin(cent, cnt, mean_dist) - db) <= 1e-12 * db


def test_host_formulas_conventions():
    cent = np.array([[0.0, 0.0], [3.0, 4.0], [9.0, 9.0]])
    assert V.calinski_harabasz(cent, [2, 2, 0], [0.0, 0.0, 0.0]) == 1.0             # W == 0
    assert V.davies_bouldin(cent, [2, 2, 0], [0.0, 0.0, 0.0]) == 0.0                # every spread 0
    assert V.davies_bouldin(cent, [2, 2, 0], [1.0, 1.5, 7.0]) == 0.5                # (1 + 1.5) / 5 for both; the empty cluster is ignored
    assert V.davies_bouldin(np.array([[1.0, 1.0], [1.0, 1.0], [4.0, 5.0]]), [2, 2, 2], [1.0, 1.0, 1.0]) == pytest.approx(0.4)   # 0 distance: 0
    # B = 2 * 6.25 + 2 * 6.25 = 25 about the mean (1.5, 2), W = 2, n = 4, k = 2
    assert V.calinski_harabasz(cent, [2, 2, 0], [1.0, 1.0, 5.0]) == pytest.approx(25.0 * 2 / (2.0 * 1))
    for fn in (V.calinski_harabasz, V.davies_bouldin):
        with pytest.raises(ValueError, match=fn.__name__ + ".*non-empty"):
            fn(cent, [4, 0, 0], [1.0, 0.0, 0.0])
        with pytest.raises(ValueError, match=fn.__name__ + ".*non-empty"):
            fn(cent, [1, 1, 1], [0.0, 0.0, 0.0])
        with pytest.raises(ValueError, match="centroids"):
            fn(cent, [1, 2], [0.0, 0.0])


# ================================================================================================ argument refusals
P4 = 4096                                                       # never dereferenced: nothing is launched


def _scan(**kw):
    a = dict(metric=0, q=P4, q_label=P4, Q=5, g=P4, seg=P4, N=7, K=3, D=4, P=2, part_a=P4, part_b=P4)
    a.update(kw)
    return L.lib().sv_sil_scan(a["metric"], a["q"], a["q_label"], a["Q"], a["g"], a["seg"], a["N"], a["K"], a["D"], a["P"], a["part_a"],
                               a["part_b"], None)


def _finish(**kw):
    a = dict(part_a=P4, part_b=P4, P=2, Q=5, q_label=P4, seg=P4, K=3, N=7, s=P4, a=None, b=None, cluster_sum=P4, cluster_cnt=P4, skipped=P4)
    a.update(kw)
    return L.lib().sv_sil_finish(a["part_a"], a["part_b"], a["P"], a["Q"], a["q_label"], a["seg"], a["K"], a["N"], a["s"], a["a"], a["b"],
                                 a["cluster_sum"], a["cluster_cnt"], a["skipped"], None)


def _spread(**kw):
    a = dict(x=P4, label=P4, N=7, D=4, c=P4, K=3, d2=P4, stat=P4, cnt=P4)
    a.update(kw)
    return L.lib().sv_cluster_spread(a["x"], a["label"], a["N"], a["D"], a["c"], a["K"], a["d2"], a["stat"], a["cnt"], None)


REFUSALS = [
    (_scan, "sv_sil_scan", [
        (dict(metric=2), b"metric"), (dict(metric=-1), b"metric"), (dict(q=None), b"NULL"), (dict(q_label=None), b"NULL"),
        (dict(g=None), b"NULL"), (dict(seg=None), b"NULL"), (dict(part_a=None), b"NULL"), (dict(part_b=None), b"NULL"),
        (dict(Q=0), b"size"), (dict(N=0), b"size"), (dict(D=-1), b"size"), (dict(K=0), b"K="), (dict(K=1025), b"K="),
        (dict(P=0), b"P="), (dict(P=65), b"P=")]),
    (_finish, "sv_sil_finish", [
        (dict(part_a=None), b"NULL"), (dict(part_b=None), b"NULL"), (dict(q_label=None), b"NULL"), (dict(seg=None), b"NULL"),
        (dict(s=None), b"NULL"), (dict(cluster_sum=None), b"together"), (dict(skipped=None), b"together"),
        (dict(cluster_cnt=None, skipped=None), b"together"), (dict(Q=0), b"size"), (dict(N=0), b"size"), (dict(K=0), b"K="),
        (dict(K=1025), b"K="), (dict(P=0), b"P="), (dict(P=65), b"P=")]),
    (_spread, "sv_cluster_spread", [
        (dict(x=None), b"NULL"), (dict(label=None), b"NULL"), (dict(c=None), b"NULL"), (dict(stat=None), b"together"),
        (dict(cnt=None), b"together"), (dict(d2=None, stat=None, cnt=None), b"no output"), (dict(N=0), b"size"), (dict(D=0), b"size"),
        (dict(K=0), b"K="), (dict(K=1025), b"K=")]),
]


@pytest.mark.parametrize("fn,name,cases", REFUSALS, ids=[r[1] for r in REFUSALS])
def test_entry_points_refuse_bad_arguments_before_any_launch(fn, name, cases):
    for kw, word in cases:
        assert fn(**kw) == SV_E_ARG, (name, kw)
        err = L.lib().sv_last_error()
        assert word in err and name.encode() in err, (kw, err)


def test_entry_points_are_bound_and_exported():
    for name in ("sv_sil_scan", "sv_sil_finish", "sv_cluster_spread"):
        assert name in L.EXPORTS and hasattr(L.lib(), name)
    assert L.lib().sv_version() == L.ABI_VERSION == 8
    for name in ("silhouette_grouped", "silhouette_samples", "silhouette_score", "cluster_spread", "calinski_harabasz", "davies_bouldin",
                 "validity_indices", "evaluate_validity"):
        assert getattr(S, name) is getattr(V, name)
    assert (L.SIL_EUCLID, L.SIL_SQEUCLID) == (R.EUCLID, R.SQEUCLID) and V.METRICS == R.METRIC


def test_python_layer_refuses_bad_arguments():
    x, y = torch.zeros(6, 3), torch.zeros(6, dtype=torch.int64)
    for fn in (V.silhouette_samples, V.silhouette_score, V.validity_indices):
        name = fn.__name__
        with pytest.raises(ValueError, match=name + ".*matrix"):
            fn(torch.zeros(6), y, 2)
        with pytest.raises(ValueError, match=name + ".*integer vector"):
            fn(x, torch.zeros(5, dtype=torch.int64), 2)
        with pytest.raises(ValueError, match=name + ".*integer vector"):
            fn(x, torch.zeros(6), 2)
        with pytest.raises(ValueError, match=name + ".*k must"):
            fn(x, y, 0)
        with pytest.raises(ValueError, match=name + ".*k must"):
            fn(x, y, 1025)
        with pytest.raises(ValueError, match=name + ".*metric"):
            fn(x, y, 2, metric="cosine")
        with pytest.raises(ValueError, match=name + ".*queries"):
            fn(x, y, 2, queries=7)
        with pytest.raises(ValueError, match=name + ".*queries"):
            fn(x, y, 2, queries=0)
    with pytest.raises(ValueError, match="cluster_spread.*matrix"):
        V.cluster_spread(torch.zeros(6), y, 2)
    seg = torch.zeros(3, dtype=torch.int64)
    for kw, word in ((dict(q=torch.zeros(6)), "matrix"), (dict(q=torch.zeros(6, 3, dtype=torch.float64)), "fp32"),
                     (dict(g=torch.zeros(4, 2)), "columns"), (dict(q_label=torch.zeros(5, dtype=torch.int64)), "q_label"),
                     (dict(q_label=torch.zeros(6, dtype=torch.int32)), "q_label"), (dict(seg=torch.zeros(2, dtype=torch.int64)), "seg"),
                     (dict(k=0), "k must"), (dict(metric="kl"), "metric"), (dict(P=0), "P must"), (dict(P=65), "P must")):
        a = dict(q=x, q_label=y, g=torch.zeros(4, 3), seg=seg, k=2)
        a.update(kw)
        with pytest.raises(ValueError, match="silhouette_grouped.*" + word):
            V.silhouette_grouped(**a)
    lin = torch.nn.Linear(2, 2)
    with pytest.raises(TypeError, match="evaluate_validity"):
        V.evaluate_validity(lin, [])


def test_cpu_tensors_are_refused():
    x, y = torch.randn(6, 3), torch.tensor([0, 0, 1, 1, 1, 0])
    seg = torch.tensor([0, 3, 6])
    for call in (lambda: V.silhouette_samples(x, y, 2), lambda: V.silhouette_score(x, y, 2, queries=3), lambda: V.validity_indices(x, y, 2),
                 lambda: V.cluster_spread(x, y, 2), lambda: V.silhouette_grouped(x, y, x, seg, 2)):
        with pytest.raises(L.ShotVaeHipError, match="MI355X"):
            call()


def test_default_partials_is_a_function_of_the_shapes():
    assert V.default_partials(10000, 10000, 10) == 10 or V.default_partials(10000, 10000, 10) >= 1
    for q, n, k in ((1, 2, 2), (65, 65, 2), (449, 449, 257), (50000, 50000, 1000)):
        p = V.default_partials(q, n, k)
        assert 1 <= p <= min(k, 64) and p == V.default_partials(q, n, k)


# ================================================================================================ the GPU tests' inputs
def _conditions(x, lab, K, name):
    sizes = np.bincount(lab, minlength=K)
    g, key, order, seg = R.grouped(x, lab, K)
    assert np.array_equal(seg[1:] - seg[:-1], sizes)
    for metric in (R.EUCLID, R.SQEUCLID):
        tol, err = R.allowance(metric, g, key, g, seg, K)
        print("FIG validity inputs %s metric=%d: allowances s %.3e a %.3e b %.3e (fp32 restatement %.3e %.3e %.3e)" % ((name, metric) + tol + err))
        assert all(np.isfinite(t) for t in tol)
    return sizes


@pytest.mark.parametrize("N,K,D", R.SHAPES_GPU)
def test_the_gpu_cases_meet_their_conditions(N, K, D):
    x, lab = R.case(N, K, D)
    sizes = _conditions(x, lab, K, "N=%d K=%d D=%d" % (N, K, D))
    assert int((sizes > 0).sum()) >= 2, "a value is expected: two non-empty clusters"
    assert sizes[0] == 1, "a singleton"
    if K >= 3:
        assert sizes[K - 1] == 0, "an empty cluster"
    if N >= 63:
        d = R.distances(R.SQEUCLID, x, x) + np.eye(N)
        i, j = np.nonzero(d == 0.0)
        assert len(i) >= 2 and lab[i[0]] == lab[j[0]], "two duplicate rows in one cluster"
        s = R.silhouette_samples(x, lab, K)
        assert np.isfinite(s).all() and s.std() > 0.01, "the silhouettes differ between the rows"


def test_the_boundary_case_has_its_exact_sizes():
    x, lab = R.boundary_case()
    sizes = _conditions(x, lab, R.BOUNDARY[1], "boundary")
    assert tuple(sizes) == R.BOUNDARY[3] == (64, 65, 129, 1, 0) and len(x) == R.BOUNDARY[0] == 259


@pytest.mark.parametrize("D", (1, 17))
def test_the_integer_cases_are_exact(D):
    """the fp32 restatement in the kernel's order equals the integer arithmetic bit for bit: no rounding anywhere before the divisions"""
    x, lab, t = R.integer_case(D)
    K = 4
    scale = 1 if D == 1 else 2
    g, key, order, seg = R.grouped(x, lab, K)
    for metric in (R.EUCLID, R.SQEUCLID):
        v32 = R.distances(metric, g, g, fp32=True)
        exact = scale * np.abs(t[order][:, None] - t[order][None, :]).astype(np.float64)
        assert np.array_equal(v32, exact * exact if metric == R.SQEUCLID else exact)
        want = R.integer_silhouette(t, scale, lab, K, metric)
        for P in (1, 3):
            got = R.finish_rows(*R.ordered_parts(metric, g, key, g, seg, K, P, V=v32), key, seg, K, len(g))
            for a, b in zip(got, want):
                assert np.array_equal(a, b[order])
        assert R.allowance(metric, g, key, g, seg, K)[0] == (0.0, 0.0, 0.0)
