"""Label spreading / propagation without a GPU: the float64 restatement of tests/_labelprop_ref.py pinned to scikit-learn and to the
closed form, its identities, the inputs of the GPU tests checked against their own conditions, the argument refusals of the three
sv_lp_* entry points (they validate before any HIP call) and the host logic of shot_vae_amd.propagate."""
import ctypes as C

import numpy as np
import pytest
import torch

import shot_vae_amd as S
from shot_vae_amd import _lib as L
from shot_vae_amd import propagate as PG
from tests import _labelprop_ref as R

SV_E_ARG = -1
# (N, D, k, K, labels per class): the blob cases of the parity tests and of the GPU fit tests
CASES = [(200, 5, 7, 3, 4), (512, 16, 10, 10, 4), (193, 33, 5, 17, 2)]
SEED = 9303          # a seed under which no iteration's delta_l1 lies within 1e-5 of tol = 1e-3 (checked below): n_iter_ is robust


def case(N, D, k, K, per):
    x, cls = R.blobs(N, D, K, SEED)
    y = R.few_labels(cls, K, per, SEED + 1)
    w = R.dense_graph(R.knn_lists(x, k)[1])
    return x, cls, y, w


# ================================================================================================ against scikit-learn
@pytest.mark.parametrize("N,D,k,K,per", CASES)
def test_the_restatement_is_scikit_learns(N, D, k, K, per):
    ss = pytest.importorskip("sklearn.semi_supervised")
    x, cls, y, w = case(N, D, k, K, per)
    assert np.array_equal(w, w.T) and not w.diagonal().any()
    runs = [("spreading 0.2", ss.LabelSpreading(kernel=lambda a, b: w, alpha=0.2), R.SYM, R.SPREADING, 0.2, 30),
            ("spreading 0.9", ss.LabelSpreading(kernel=lambda a, b: w, alpha=0.9, max_iter=1000), R.SYM, R.SPREADING, 0.9, 1000),
            ("propagation", ss.LabelPropagation(kernel=lambda a, b: w, max_iter=1000), R.ROW, R.PROPAGATION, 0.0, 1000)]
    for name, sk, mode, variant, alpha, max_iter in runs:
        sk.fit(x, y)
        f, n_iter, converged, _ = R.iterate(R.normalize(w, mode), y, K, variant, alpha, max_iter, 1e-3)
        proba, pred, _, _ = R.finish(f)
        err = float(np.abs(proba - sk.label_distributions_).max())
        print("FIG scikit-learn %s %s: label_distributions_ %.1e, n_iter %d / %d" % ((N, D, k, K, per), name, err, n_iter, sk.n_iter_))
        assert err <= 1e-12
        assert n_iter == sk.n_iter_ and converged
        assert np.array_equal(pred, sk.transduction_)


@pytest.mark.parametrize("alpha", [0.2, 0.9])
def test_spreading_converges_to_the_closed_form(alpha):
    for N, D, k, K, per in CASES:
        x, cls, y, w = case(N, D, k, K, per)
        s = R.normalize(w, R.SYM)
        f, n_iter, converged, _ = R.iterate(s, y, K, R.SPREADING, alpha, 5000, 1e-13)
        err = float(np.abs(f - R.closed_form(s, y, K, alpha)).max())
        print("FIG closed form %s alpha=%g: %.1e after %d iterations" % ((N, D, k, K, per), alpha, err, n_iter))
        assert converged and err <= 1e-10


# ================================================================================================ identities
def two_components():
    """rows 0..4 a path, rows 5..8 a cycle, row 9 isolated and unlabelled, row 10 isolated and labelled"""
    w = np.zeros((11, 11))
    for a, b in ((0, 1), (1, 2), (2, 3), (3, 4), (5, 6), (6, 7), (7, 8), (8, 5)):
        w[a, b] = w[b, a] = 1.0
    y = np.full(11, -1, dtype=np.int64)
    y[0], y[6], y[10] = 0, 1, 2
    return w, y


@pytest.mark.parametrize("variant,mode", [(R.SPREADING, R.SYM), (R.PROPAGATION, R.ROW)])
def test_isolated_rows_and_disconnected_components(variant, mode):
    w, y = two_components()
    s = R.normalize(w, mode)
    assert np.isfinite(s).all() and not s[9].any() and not s[10].any()
    f, _, _, _ = R.iterate(s, y, 3, variant, 0.5, 200, 1e-15)
    proba, pred, _, (decided, unreached) = R.finish(f)
    assert not f[9].any() and pred[9] == -1 and unreached == 1 and decided == 10
    want = (0.5 if variant == R.SPREADING else 1.0) * np.array([0, 0, 1.0])
    assert np.abs(f[10] - want).max() <= 1e-15 and pred[10] == 2
    # no mass crosses between the components
    assert not f[:5, 1:].any() and not f[5:9, 0].any() and not f[5:9, 2].any()
    assert (pred[:5] == 0).all() and (pred[5:9] == 1).all()
    # the same through the CSR form, from fp32 storage
    rowptr, col, val = R.to_csr(w)
    sval, deg = R.csr_normalize(rowptr, col, val, 11, mode)
    assert np.array_equal(deg, w.sum(axis=1)) and np.isfinite(sval).all()
    g, _, _, _ = R.csr_iterate(rowptr, col, sval, y, 11, 3, variant, 0.5, 200, 0.0)
    assert not g[9].any() and not g[:5, 1:].any() and not g[5:9, 0].any() and np.abs(g - f).max() <= 1e-6
    assert np.array_equal(R.csr_finish(g)[1], pred) and R.csr_finish(g)[3] == (10, 1)


def test_the_scale_of_symmetrize_changes_nothing():
    N, D, k, K, per = CASES[0]
    x, cls, y, _ = case(N, D, k, K, per)
    idx = R.knn_lists(x, k)[1]
    a, b = R.dense_graph(idx), R.dense_graph(idx, scaled=False)
    assert np.abs(a * 2 * N - b).max() == 0
    for mode in (R.SYM, R.ROW):
        assert np.abs(R.normalize(a, mode) - R.normalize(b, mode)).max() <= 1e-15


def test_the_product_on_a_connectivity_graph_counts_the_neighbours_labels():
    N, D, k, K, per = CASES[0]
    x, cls, y, _ = case(N, D, k, K, per)
    w = R.dense_graph(R.knn_lists(x, k)[1], scaled=False)
    w = (w > 0).astype(np.float64)
    rowptr, col, val = R.to_csr(w)
    out = R.csr_step(rowptr, col, val, R.one_hot(cls, K), N, K, None, R.PRODUCT)
    want = np.stack([np.bincount(cls[np.nonzero(w[i])[0]], minlength=K) for i in range(N)])
    assert np.array_equal(out, want) and np.array_equal(R.step(w, R.one_hot(cls, K), None, R.PRODUCT), want)


def test_the_csr_form_follows_the_dense_form():
    N, D, k, K, per = CASES[2]
    x, cls, y, w = case(N, D, k, K, per)
    rowptr, col, val = R.to_csr(w)
    for mode, variant in ((R.SYM, R.SPREADING), (R.ROW, R.PROPAGATION)):
        sval, deg = R.csr_normalize(rowptr, col, val, N, mode)
        s = R.normalize(R.to_dense(rowptr, col, val, N), mode)
        assert np.abs(R.to_dense(rowptr, col, sval, N) - s).max() <= R.EPS32 * np.abs(s).max()
        f = R.one_hot(y, K)
        for _ in range(3):
            g = R.csr_step(rowptr, col, sval, f, N, K, y, variant, 0.2)
            assert np.abs(g - R.step(s, f, y, variant, 0.2)).max() <= 4 * R.EPS32
            f = g


def fit_case(N, D, k, K, per, variant):
    """a blob case as the GPU test fits it -> everything both sides need (see test_labelprop_gpu.test_fit_follows_the_restatement)"""
    x, cls, y, w = case(N, D, k, K, per)
    mode = R.SYM if variant == R.SPREADING else R.ROW
    rowptr, col, val = R.to_csr(w)
    s = R.normalize(R.to_dense(rowptr, col, val, N), mode)
    max_iter = 30 if variant == R.SPREADING else 1000
    f64, n64, conv64, deltas = R.iterate(s, y, K, variant, 0.2, max_iter, 1e-3, 10)
    return dict(x=x, cls=cls, y=y, rowptr=rowptr, col=col, val=val, s=s, f64=f64, n_iter=n64, converged=conv64, deltas=deltas,
                max_iter=max_iter)


@pytest.mark.parametrize("variant", [R.SPREADING, R.PROPAGATION])
@pytest.mark.parametrize("N,D,k,K,per", CASES)
def test_the_inputs_of_the_gpu_fit_tests_meet_their_conditions(N, D, k, K, per, variant):
    """the float64 margin leaves at most 2 % of the rows undecided at the fp32 restatement's allowance, and no iteration's delta_l1
    is within 1e-5 of the stopping threshold -- conditions on the INPUTS, checked where no GPU is needed"""
    c = fit_case(N, D, k, K, per, variant)
    f32, n32, _, _ = R.iterate(c["s"], c["y"], K, variant, 0.2, c["max_iter"], 1e-3, 10, np.float32)
    p64, p32 = R.finish(c["f64"])[0], R.finish(f32)[0]
    tol = R.allowance(p32, p64)
    undecided = int((R.margin(p64) <= 2.0 * tol).sum())
    print("FIG fit inputs %s variant %d: n_iter %d (fp32 %d), allowance %.2e, undecided rows %d of %d"
          % ((N, D, k, K, per), variant, c["n_iter"], n32, tol, undecided, N))
    assert undecided <= 0.02 * N
    assert n32 == c["n_iter"]
    assert all(abs(d - 1e-3) > 1e-5 for d in c["deltas"])         # (the fp32 restatement's deltas differ from these by < 1e-6)


# ================================================================================================ the stopping rule
def scripted(values, **kw):
    reads, it = [], iter(values)
    def read(handle):
        reads.append(handle)
        return handle
    n, conv, delta = PG._lp_loop(lambda: next(it), read, **kw)
    return n, conv, reads


def test_fit_stops_by_scikit_learns_rule_on_a_scripted_sequence():
    seq = [1.0, 0.1, 1e-5, 0.5, 1e-6, 1e-7]
    assert scripted(seq, max_iter=6, tol=1e-3, check_every=1) == (3, True, [1.0, 0.1, 1e-5])
    assert scripted(seq, max_iter=6, tol=1e-3, check_every=2) == (6, False, [0.1, 0.5])            # the last product is never looked at
    assert scripted(seq, max_iter=3, tol=1e-3, check_every=1) == (3, False, [1.0, 0.1])
    assert scripted(seq, max_iter=6, tol=1e-3, check_every=5) == (5, True, [1e-6])
    assert scripted(seq, max_iter=6, tol=1e-3, check_every=7) == (6, False, [])
    assert scripted([float("nan")] * 3, max_iter=3, tol=1e-3, check_every=1)[:2] == (3, False)     # a NaN never converges
    assert scripted([1e-3, 1e-3], max_iter=2, tol=1e-3, check_every=1)[:2] == (2, False)           # strictly below tol
    # the restatement's loop is the same rule
    for ce in (1, 2, 5, 7):
        it = iter(seq)
        want = PG._lp_loop(lambda: next(it), lambda h: h, 6, 1e-3, ce)[:2]
        n, conv = next(((t, True) for t, d in enumerate(seq, 1) if t % ce == 0 and t < 6 and d < 1e-3), (6, False))
        assert want == (n, conv)


# ================================================================================================ the entry points' refusals
P4 = C.c_void_p(4096)               # never dereferenced: nothing is launched
P8 = C.c_void_p(1 << 20)


def _normalize(**kw):
    a = dict(rowptr=P4, col=P4, val=P4, N=5, nnz=7, mode=0, deg=P4, sval=P4)
    a.update(kw)
    return L.lib().sv_lp_normalize(a["rowptr"], a["col"], a["val"], a["N"], a["nnz"], a["mode"], a["deg"], a["sval"], None)


def _step(**kw):
    a = dict(f_in=P4, M=5, rowptr=P4, col=P4, sval=P4, nnz=7, N=5, K=3, label=P4, variant=0, alpha=0.2, oma=0.8, f_out=P8, scratch=P4, stats=P4)
    a.update(kw)
    return L.lib().sv_lp_step(a["f_in"], a["M"], a["rowptr"], a["col"], a["sval"], a["nnz"], a["N"], a["K"], a["label"], a["variant"],
                              a["alpha"], a["oma"], a["f_out"], a["scratch"], a["stats"], None)


def _finish(**kw):
    a = dict(f=P4, N=5, K=3, proba=P8, pred=P4, conf=P4, counts=P4)
    a.update(kw)
    return L.lib().sv_lp_finish(a["f"], a["N"], a["K"], a["proba"], a["pred"], a["conf"], a["counts"], None)


REFUSALS = [
    (_normalize, "sv_lp_normalize", [(dict(rowptr=None), b"NULL"), (dict(col=None), b"NULL"), (dict(val=None), b"NULL"), (dict(sval=None), b"NULL"),
                                     (dict(deg=None), b"NULL"), (dict(N=0), b"size"), (dict(N=-3), b"size"), (dict(nnz=-1), b"size"),
                                     (dict(mode=2), b"mode"), (dict(mode=-1), b"mode")]),
    (_step, "sv_lp_step", [(dict(f_in=None), b"NULL"), (dict(f_out=None), b"NULL"), (dict(rowptr=None), b"NULL"), (dict(col=None), b"NULL"),
                           (dict(sval=None), b"NULL"), (dict(label=None), b"label"), (dict(label=None, variant=1), b"label"),
                           (dict(N=0), b"size"), (dict(N=-1), b"size"), (dict(M=0), b"size"), (dict(nnz=-1), b"size"), (dict(K=0), b"K=0"),
                           (dict(K=1025), b"K=1025"), (dict(K=-2), b"K=-2"), (dict(variant=3), b"variant"), (dict(variant=-1), b"variant"),
                           (dict(f_out=P4), b"aliases"), (dict(f_out=C.c_void_p(4096 + 8)), b"aliases"),
                           (dict(f_in=C.c_void_p((1 << 20) + 16)), b"aliases"), (dict(alpha=float("nan")), b"finite"),
                           (dict(oma=float("inf")), b"finite"), (dict(scratch=None), b"scratch"), (dict(M=6), b"M == N")]),
    (_finish, "sv_lp_finish", [(dict(f=None), b"NULL"), (dict(N=0), b"size"), (dict(N=-1), b"size"), (dict(K=0), b"K=0"), (dict(K=1025), b"K=1025"),
                               (dict(proba=None, pred=None, conf=None, counts=None), b"NULL"), (dict(proba=P4), b"aliases")]),
]


@pytest.mark.parametrize("fn,name,cases", REFUSALS, ids=[r[1] for r in REFUSALS])
def test_entry_points_refuse_bad_arguments_before_any_launch(fn, name, cases):
    for kw, word in cases:
        assert fn(**kw) == SV_E_ARG, (name, kw)
        err = L.lib().sv_last_error()
        assert word in err and name.encode() in err, (kw, err)


def test_entry_points_are_bound_and_exported():
    for name in ("sv_lp_normalize", "sv_lp_step", "sv_lp_finish"):
        assert name in L.EXPORTS and hasattr(L.lib(), name)
    assert L.lib().sv_version() == L.ABI_VERSION == 8
    for name in ("LabelPropagator", "knn_graph", "normalize_graph", "evaluate_propagation"):
        assert getattr(S, name) is getattr(PG, name)
    assert (L.LP_SYM, L.LP_ROW) == (R.SYM, R.ROW) and (L.LP_SPREADING, L.LP_PROPAGATION, L.LP_PRODUCT) == (R.SPREADING, R.PROPAGATION, R.PRODUCT)


# ================================================================================================ host logic
def test_scratch_size_follows_the_kernels_blocks():
    assert PG.step_scratch(1, 1) == 2 and PG.step_scratch(16, 16) == 2 and PG.step_scratch(17, 16) == 4
    assert PG.step_scratch(4, 17) == 2 and PG.step_scratch(5, 17) == 4 and PG.step_scratch(50000, 10) == 2 * 3125
    assert PG.step_scratch(50000, 100) == 2 * 12500


def test_python_layer_refuses_bad_arguments():
    for bad in (dict(num_classes=0), dict(num_classes=1025), dict(num_classes=3, variant="harmonic"), dict(num_classes=3, alpha=0.0),
                dict(num_classes=3, alpha=1.0), dict(num_classes=3, max_iter=0), dict(num_classes=3, tol=-1.0),
                dict(num_classes=3, metric="cosine"), dict(num_classes=3, weights="rbf"), dict(num_classes=3, k=0), dict(num_classes=3, k=257)):
        with pytest.raises(ValueError):
            S.LabelPropagator(**bad)
    assert S.LabelPropagator(3).max_iter == 30 and S.LabelPropagator(3, "propagation").max_iter == 1000
    assert S.LabelPropagator(3).k == 7 and S.LabelPropagator(3).tol == 1e-3 and S.LabelPropagator(3).alpha == 0.2
    S.LabelPropagator(3, "propagation", alpha=1.0)              # (propagation has no alpha)
    lp = S.LabelPropagator(3)
    mu, y = torch.zeros(9, 4), torch.zeros(9, dtype=torch.int64)
    for call in (lambda: lp.predict(mu), lambda: lp.predict_proba(mu)):
        with pytest.raises(ValueError, match="call fit"):
            call()
    for call in (lp.step, lp.reset, lp.finish):
        with pytest.raises(ValueError, match="prepare"):
            call()
    with pytest.raises(ValueError, match="nothing fitted"):
        lp.state_dict()
    with pytest.raises(ValueError, match="check_every"):
        lp.fit(mu, mu, y, check_every=0)
    with pytest.raises(ValueError, match="cosine"):
        S.knn_graph(mu, None, metric="cosine")
    with pytest.raises(ValueError, match="weights"):
        S.knn_graph(mu, mu, weights="rbf")
    with pytest.raises(ValueError, match="k must be"):
        S.knn_graph(mu, mu, k=9)
    with pytest.raises(ValueError, match="matrix"):
        S.knn_graph(mu.view(-1), None)
    with pytest.raises(ValueError, match="mode"):
        S.normalize_graph(torch.zeros(3, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), torch.zeros(0), mode="col")
    with pytest.raises(ValueError, match="rowptr"):
        S.normalize_graph(torch.zeros(3), torch.zeros(0, dtype=torch.int64), torch.zeros(0))
    with pytest.raises(TypeError):
        S.evaluate_propagation(object(), [])


def test_cpu_tensors_are_refused():
    lp = S.LabelPropagator(3, k=2)
    mu, y = torch.zeros(9, 4), torch.zeros(9, dtype=torch.int64)
    rowptr, col, val = torch.arange(10), torch.arange(9), torch.ones(9)
    for call in (lambda: lp.fit(mu, mu, y), lambda: lp.prepare(mu, mu, y), lambda: S.knn_graph(mu, mu, k=2),
                 lambda: S.normalize_graph(rowptr, col, val), lambda: lp.prepare_graph(rowptr, col, val, y)):
        with pytest.raises(L.ShotVaeHipError, match="MI355X"):
            call()
    # a state loaded onto the host is refused at its first use
    sd = dict(num_classes=3, variant="spreading", alpha=0.2, max_iter=30, tol=1e-3, k=2, metric="euclid", weights="connectivity", perplexity=None,
              label_distributions=torch.full((9, 3), 1 / 3), transduction=torch.zeros(9, dtype=torch.int64), mu=mu, ls=None, n_iter=7,
              converged=True, delta=5e-4, n_unreached=0)
    lp.load_state_dict(sd)
    assert lp.n_iter_ == 7 and lp.converged_ is True and lp.metric == "euclid"
    with pytest.raises(L.ShotVaeHipError, match="MI355X"):
        lp.predict(mu)
    out = lp.state_dict()
    assert torch.equal(out["label_distributions"], sd["label_distributions"]) and out["label_distributions"] is not lp.label_distributions_
    assert torch.equal(out["mu"], mu) and out["ls"] is None and out["n_iter"] == 7
    with pytest.raises(ValueError, match="classes"):
        S.LabelPropagator(4).load_state_dict(sd)
    with pytest.raises(ValueError, match="rows"):
        S.LabelPropagator(3).load_state_dict(dict(sd, mu=torch.zeros(8, 4)))
    with pytest.raises(ValueError, match=r"matrix \[Q"):
        lp.predict(torch.zeros(2, 5))
