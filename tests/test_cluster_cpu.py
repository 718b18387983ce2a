"""Latent-space clustering without a GPU: the float64 restatement of tests/_cluster_ref.py and the package's host formulas
(shot_vae_amd.cluster.partition_metrics, linear_assignment) against scikit-learn and scipy where they are installed and always
against brute force and identities whose answer is known; the argument refusals of the four entry points of csrc/cluster.hip through
the library; the Python layer's errors.

One identity of the issue is not asserted as it was worded: an independent (product) table does NOT have an adjusted Rand index of
exactly 0 -- r = c = (10, 10) gives 19800 agreeing pairs against an expectation of 39800^2 / 79800 = 19850.1, ARI = -0.0025.  What
holds exactly is: its mutual information, NMI, homogeneity and completeness are 0, and a single block against any partition has ARI
exactly 0 (the index equals its expectation term by term).  Both are asserted, and the product table's ARI is compared with the pair
count by brute force."""
import itertools

import numpy as np
import pytest
import torch

import shot_vae_amd as S
from shot_vae_amd import _lib as L
from shot_vae_amd import cluster as CL
from oracle import smooth_oracle as SO
from tests import _cluster_ref as R

SV_E_ARG, SV_E_SHAPE = -1, -2    # include/shotvae_hip.h
PTR = 4096                       # never dereferenced: a refused call launches nothing
FLOATS = ("accuracy", "purity", "nmi", "ari", "homogeneity", "completeness", "v_measure")


def tables():
    rng = np.random.RandomState(5101)
    out = [rng.randint(0, 9, size=s) for s in ((2, 2), (3, 3), (4, 6), (6, 4), (1, 5), (5, 1), (6, 6), (3, 7))]
    out.append(np.array([[5, 0, 0], [0, 0, 0], [0, 3, 2]]))                      # an empty row
    out.append(np.array([[5, 0, 1], [2, 0, 4], [0, 0, 2]]))                      # an empty column
    out.append(np.diag([4, 1, 7, 2]))
    return [t for t in out if t.sum() > 1]


def labels_of(table):
    """two label vectors with this contingency table"""
    a, b = [], []
    for i in range(table.shape[0]):
        for j in range(table.shape[1]):
            a += [i] * int(table[i, j])
            b += [j] * int(table[i, j])
    return np.array(a), np.array(b)


def rand_index_by_pairs(a, b):
    """ARI from the definition: count every pair of rows"""
    n = len(a)
    tp = fp = fn = tn = 0
    for i, j in itertools.combinations(range(n), 2):
        sa, sb = a[i] == a[j], b[i] == b[j]
        tp += sa and sb
        fn += sa and not sb
        fp += sb and not sa
        tn += not sa and not sb
    if fn == 0 and fp == 0:
        return 1.0
    return 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))


# ================================================================================================ the metrics
@pytest.mark.parametrize("fn", [R.metrics, CL.partition_metrics])
def test_metrics_match_scikit_learn(fn):
    M = pytest.importorskip("sklearn.metrics")
    for t in tables():
        a, b = labels_of(t)
        got = fn(t)
        h, c, v = M.homogeneity_completeness_v_measure(a, b)
        want = dict(nmi=M.normalized_mutual_info_score(a, b, average_method="arithmetic"), ari=M.adjusted_rand_score(a, b), homogeneity=h,
                    completeness=c, v_measure=v)
        for name, w in want.items():
            assert abs(got[name] - w) <= 1e-12, (name, t.tolist(), got[name], w)


def test_linear_assignment_matches_scipy():
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    rng = np.random.RandomState(5103)
    for shape in ((1, 1), (5, 5), (3, 7), (7, 3), (1, 4), (20, 20), (40, 13), (13, 40), (64, 64)):
        c = rng.randn(*shape)                              # no ties: the assignment is unique
        r, cc = S.linear_assignment(c)
        r2, c2 = lsa(c)
        assert np.array_equal(r, r2) and np.array_equal(cc, c2), shape
        c = rng.randint(0, 6, size=shape).astype(np.float64)          # many ties: the same cost
        r, cc = S.linear_assignment(c)
        assert len(set(cc.tolist())) == len(cc) == min(shape) and (np.diff(r) > 0).all()
        assert c[r, cc].sum() == c[lsa(c)].sum(), shape


def test_package_and_restatement_agree_with_brute_force():
    for t in tables():
        got, ref = CL.partition_metrics(t), R.metrics(t)
        assert got["n"] == ref["n"] == int(t.sum())
        for name in FLOATS:
            assert abs(got[name] - ref[name]) <= 1e-12, (name, t.tolist())
        assert got["accuracy"] == R.best_matching(t) / got["n"]
        # the mapping is one-to-one and attains the accuracy
        m = got["mapping"]
        used = m[m >= 0]
        assert len(set(used.tolist())) == len(used) == min(t.shape) and m.shape == (t.shape[1],)
        assert sum(int(t[m[j], j]) for j in range(t.shape[1]) if m[j] >= 0) == R.best_matching(t)
        a, b = labels_of(t)
        if len(a) <= 60:
            assert abs(got["ari"] - rand_index_by_pairs(a, b)) <= 1e-12
    rng = np.random.RandomState(5105)
    for shape in ((2, 5), (5, 2), (6, 6), (4, 3)):
        cost = rng.randint(0, 20, size=shape)
        r, c = S.linear_assignment(-cost)
        assert cost[r, c].sum() == R.best_matching(cost)
        assert R.best_matching_dp(cost) == R.best_matching(cost)
    for shape in ((10, 10), (12, 9), (3, 11)):                  # beyond the permutations: the subset recursion
        cost = rng.randint(0, 20, size=shape)
        r, c = S.linear_assignment(-cost)
        assert cost[r, c].sum() == R.best_matching_dp(cost)


@pytest.mark.parametrize("fn", [R.metrics, CL.partition_metrics])
def test_identities(fn):
    # identical partitions up to a relabelling
    perm = [2, 0, 3, 1]
    t = np.zeros((4, 4), dtype=np.int64)
    for i, n in enumerate((5, 1, 7, 3)):
        t[i, perm[i]] = n
    got = fn(t)
    exact = 0.0 if fn is CL.partition_metrics else 1e-15      # (the package decides the perfect cases on the integers)
    assert got["accuracy"] == got["ari"] == got["purity"] == 1.0
    assert all(abs(got[name] - 1.0) <= exact for name in ("nmi", "homogeneity", "completeness", "v_measure"))
    if "mapping" in got:
        assert [int(got["mapping"][perm[i]]) for i in range(4)] == [0, 1, 2, 3]
    # one cluster against many classes, and many clusters against one class: ARI exactly 0
    one = fn(np.array([[4], [2], [6], [1]]))
    assert one["ari"] == 0.0 and one["nmi"] == 0.0 and one["completeness"] == 1.0 and one["homogeneity"] == 0.0 and one["v_measure"] == 0.0
    assert one["accuracy"] == one["purity"] == 6 / 13
    many = fn(np.array([[4, 2, 6, 1]]))
    assert many["ari"] == 0.0 and many["nmi"] == 0.0 and many["homogeneity"] == 1.0 and many["completeness"] == 0.0
    assert many["accuracy"] == 6 / 13 and many["purity"] == 1.0
    # a single block on both sides
    both = fn(np.array([[9]]))
    assert both["ari"] == both["nmi"] == both["accuracy"] == both["v_measure"] == 1.0
    # an independent product table: no information (see the module's docstring for its ARI)
    for r, c in (((10, 10), (10, 10)), ((1, 2, 3), (4, 1)), ((2, 5), (3, 3, 1))):
        t = np.outer(r, c)
        got = fn(t)
        # every term is weight x (log t + log n - log(a b)) = weight x 0 up to the roundings of three logarithms of size <= log(400) ~ 6
        # (<= 6 x 2^-53 each plus two additions: <= 4e-15 per unit of weight, the weights sum to 1); the entropies that divide are >= 0.5
        assert abs(got["nmi"]) <= 1e-14 and abs(got["homogeneity"]) <= 1e-14 and abs(got["completeness"]) <= 1e-14
        if t.sum() <= 60:
            assert abs(got["ari"] - rand_index_by_pairs(*labels_of(t))) <= 1e-12
    assert abs(fn(np.outer((10, 10), (10, 10)))["ari"] - (19800 - 39800 ** 2 / 79800) / (39800 - 39800 ** 2 / 79800)) <= 1e-12
    # empty rows and columns change nothing
    base = np.array([[5, 1], [2, 6]])
    padded = np.array([[5, 0, 1], [0, 0, 0], [2, 0, 6]])
    g0, g1 = fn(base), fn(padded)
    for name in FLOATS:
        assert abs(g0[name] - g1[name]) <= 1e-15, name


def test_partition_metrics_refuses_bad_tables():
    for bad in (np.zeros((2, 2)), np.array([[1, -1]]), np.zeros(3), np.zeros((0, 2))):
        with pytest.raises(ValueError):
            S.partition_metrics(bad)
    with pytest.raises(ValueError, match="finite"):
        S.linear_assignment(np.array([[np.nan]]))


# ================================================================================================ the restatement itself
def test_restatement_assignment_and_update_rules():
    x = np.array([[0.0, 0.0], [4.0, 0.0], [2.0, 0.0], [np.nan, 0.0], [np.inf, 1.0]])
    c = np.array([[0.0, 0.0], [4.0, 0.0], [9.0, 9.0]])
    a, v = R.assign(x, c)
    assert a.tolist() == [0, 1, 0, -1, -1]                  # the tie of row 2 goes to the smaller index
    assert v[:3].tolist() == [0.0, 0.0, 4.0] and np.isinf(v[3:]).all()
    assert R.assign(x[:3], np.full((2, 2), np.nan))[0].tolist() == [-1, -1, -1]
    c_new, count, _, inertia = R.update(x, a, c, v)
    assert count.tolist() == [2, 1, 0] and c_new.tolist() == [[1.0, 0.0], [4.0, 0.0], [9.0, 9.0]] and inertia == 4.0
    assert R.shift(c_new, c) == 1.0
    t, counts = R.contingency(np.array([0, 1, 5, -1, 1]), np.array([2, 0, 0, 1, 0]), 2, 3)
    assert t.tolist() == [[0, 0, 1], [2, 0, 0]] and counts.tolist() == [3, 5]


def test_restatement_seeding_draws_distinct_rows():
    x, _, _ = R.blobs(40, 5, 3, 5107)
    for seed in range(4):
        u = np.random.RandomState(seed).uniform(size=5)
        idx = R.plus_plus(x, 5, u)
        assert len(set(idx.tolist())) == 5 and idx[0] == int(u[0] * 40)
    assert R.plus_plus(x, 3, np.array([0.0, 0.0, 0.999999])).tolist()[0] == 0


# ================================================================================================ argument refusals
def _assign(**kw):
    a = dict(x=PTR, N=5, c=PTR, K=3, D=7, assign=PTR, dist=PTR)
    a.update(kw)
    return L.lib().sv_kmeans_assign(a["x"], a["N"], a["c"], a["K"], a["D"], a["assign"], a["dist"], None)


def _accum(**kw):
    a = dict(x=PTR, assign=PTR, dist=PTR, N=5, D=7, K=3, sums=PTR, counts=PTR, inertia=PTR, P=2, init=1)
    a.update(kw)
    return L.lib().sv_kmeans_accum(a["x"], a["assign"], a["dist"], a["N"], a["D"], a["K"], a["sums"], a["counts"], a["inertia"], a["P"],
                                   a["init"], None)


def _finish(**kw):
    a = dict(sums=PTR, counts=PTR, inertia=PTR, P=2, K=3, D=7, c_old=PTR, c_new=PTR, count=PTR, stats=PTR)
    a.update(kw)
    return L.lib().sv_kmeans_finish(a["sums"], a["counts"], a["inertia"], a["P"], a["K"], a["D"], a["c_old"], a["c_new"], a["count"],
                                    a["stats"], None)


def _table(**kw):
    a = dict(a=PTR, b=PTR, N=5, Ka=3, Kb=4, table=PTR, counts=PTR)
    a.update(kw)
    return L.lib().sv_contingency(a["a"], a["b"], a["N"], a["Ka"], a["Kb"], a["table"], a["counts"], None)


SIZES = (0, -3)


@pytest.mark.parametrize("fn,name,cases", [
    (_assign, b"sv_kmeans_assign",
     [(dict(x=None), SV_E_ARG, b"NULL"), (dict(c=None), SV_E_ARG, b"NULL"), (dict(assign=None), SV_E_ARG, b"NULL")]
     + [(dict([(k, v)]), SV_E_ARG, b"size") for k in ("N", "K", "D") for v in SIZES]),
    (_accum, b"sv_kmeans_accum",
     [(dict([(k, None)]), SV_E_ARG, b"NULL") for k in ("x", "assign", "sums", "counts")]
     + [(dict(dist=None), SV_E_ARG, b"needs dist")]
     + [(dict([(k, v)]), SV_E_ARG, b"size") for k in ("N", "K", "D") for v in SIZES]
     + [(dict(K=1025), SV_E_ARG, b"K=1025"), (dict(P=0), SV_E_ARG, b"P=0"), (dict(P=65), SV_E_ARG, b"P=65"), (dict(P=-1), SV_E_ARG, b"P=-1")]),
    (_finish, b"sv_kmeans_finish",
     [(dict([(k, None)]), SV_E_ARG, b"NULL") for k in ("sums", "counts", "c_old", "c_new", "count", "stats")]
     + [(dict([(k, v)]), SV_E_ARG, b"size") for k in ("K", "D") for v in SIZES]
     + [(dict(P=0), SV_E_ARG, b"P=0"), (dict(P=65), SV_E_ARG, b"P=65")]),
    (_table, b"sv_contingency",
     [(dict([(k, None)]), SV_E_ARG, b"NULL") for k in ("a", "b", "table", "counts")]
     + [(dict([(k, v)]), SV_E_ARG, b"size") for k in ("N", "Ka", "Kb") for v in SIZES]
     + [(dict(Ka=1025, Kb=1024), SV_E_SHAPE, b"2^20"), (dict(Ka=2 ** 20 + 1, Kb=1), SV_E_SHAPE, b"2^20"),
        (dict(Ka=2 ** 30, Kb=2 ** 30), SV_E_SHAPE, b"2^20")]),
])
def test_entry_points_refuse_bad_arguments_before_any_launch(fn, name, cases):
    for kw, code, word in cases:
        assert fn(**kw) == code, (name, kw)
        err = L.lib().sv_last_error()
        assert word in err and name in err, (kw, err)


def test_entry_points_are_bound_and_exported():
    for name in ("sv_kmeans_assign", "sv_kmeans_accum", "sv_kmeans_finish", "sv_contingency"):
        assert name in L.EXPORTS and hasattr(L.lib(), name)
    assert L.lib().sv_version() == L.ABI_VERSION == 8
    for name in ("KMeans", "kmeans_plus_plus", "contingency", "linear_assignment", "partition_metrics", "evaluate_clustering"):
        assert getattr(S, name) is getattr(CL, name)


# ================================================================================================ the Python layer
def test_python_layer_refuses_cpu_tensors_and_bad_arguments():
    x = torch.zeros(6, 8)
    for bad in (0, -1, 1025):
        with pytest.raises(ValueError, match="k must be"):
            S.KMeans(bad, 8)
    with pytest.raises(ValueError, match="dim must be"):
        S.KMeans(2, 0)
    with pytest.raises(ValueError, match="init must be"):
        S.KMeans(2, 8, init="farthest")
    for shape in ((2, 7), (3, 8), (16,)):
        with pytest.raises(ValueError, match="init must be a tensor"):
            S.KMeans(2, 8, init=torch.zeros(shape))
    with pytest.raises(L.ShotVaeHipError, match="MI355X"):
        S.KMeans(2, 8, init=torch.zeros(2, 8))
    km = S.KMeans(2, 8)
    for call in (lambda: km.fit(x), lambda: km.step(x), lambda: km.predict(x), lambda: S.kmeans_plus_plus(x, 2, torch.zeros(2, dtype=torch.float64))):
        with pytest.raises(L.ShotVaeHipError, match="MI355X|no CPU fallback"):
            call()
    with pytest.raises(L.ShotVaeHipError, match="MI355X"):
        S.contingency(torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int64), 2, 2)
    assert km.centroids is None and km.n_iter == 0


def test_python_layer_checks_shapes_before_it_asks_for_the_device():
    x = torch.zeros(6, 8)
    with pytest.raises(ValueError, match="k > N"):
        S.KMeans(7, 8).fit(x)
    with pytest.raises(ValueError, match="k > N"):
        S.KMeans(7, 8, init="random").fit(x)
    with pytest.raises(ValueError, match="k > N"):
        S.kmeans_plus_plus(x, 7, torch.zeros(7, dtype=torch.float64))
    with pytest.raises(ValueError, match="columns"):
        S.KMeans(2, 5).fit(x)
    with pytest.raises(ValueError, match=">= 1"):
        S.KMeans(2, 8).fit(x, max_iter=0)
    with pytest.raises(ValueError, match="matrix"):
        S.KMeans(2, 8).fit(x.view(-1))
    for a, b, ka, kb in ((torch.zeros(4), torch.zeros(4), 2, 2), (torch.zeros(4, dtype=torch.int64), torch.zeros(3, dtype=torch.int64), 2, 2)):
        with pytest.raises((ValueError, L.ShotVaeHipError)):
            S.contingency(a, b, ka, kb)


def test_evaluate_clustering_is_eval_mode_only_and_checks_its_arguments():
    x, y = torch.zeros(2, 3, 32, 32), torch.zeros(2, dtype=torch.int64)
    vae = S.VariationalAutoEncoder("wideresnet-10-1", num_input_channels=3, img_size=(32, 32), data_parallel=False,
                                   continuous_latent_dim=128, disc_latent_dim=10, small_input=True, compute_dtype="fp32")
    smooth = S.SmoothVAE((SO.KINDS["svhn"]["in_ch"], 32, 32), {"cont": 32, "disc": [10]}, compute_dtype="fp32")
    for m in (vae, smooth):
        m.train()
        for method in ("posterior", "kmeans"):
            with pytest.raises(NotImplementedError, match="eval mode only"):
                S.evaluate_clustering(m, [(x, y)], method=method)
        m.eval()
        with pytest.raises(L.ShotVaeHipError, match="MI355X"):
            S.evaluate_clustering(m, [(x, y)])
        with pytest.raises(ValueError, match="empty"):
            S.evaluate_clustering(m, [])
        with pytest.raises(ValueError, match=r"\(image, label\)"):
            S.evaluate_clustering(m, [x])
        for kw, word in ((dict(method="spectral"), "method"), (dict(space="features"), "space"), (dict(k=3), "takes no k"),
                         (dict(seed=1), "takes no k")):
            with pytest.raises(ValueError, match=word):
                S.evaluate_clustering(m, [(x, y)], **kw)
        assert not m.training
    with pytest.raises(TypeError, match="VariationalAutoEncoder or a SmoothVAE"):
        S.evaluate_clustering(torch.nn.Linear(2, 2), [(x, y)])
