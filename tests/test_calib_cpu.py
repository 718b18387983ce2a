"""Calibration, temperature scaling and detection metrics without a GPU: the float64 restatement of tests/_calib_ref.py against
scikit-learn and scipy where they are installed and always against hand-counted cases and identities whose answer is known; the
argument refusals of the six entry points of csrc/calib.hip through the library; the Python layer's errors."""
import numpy as np
import pytest
import torch

import shot_vae_amd as S
from shot_vae_amd import _lib as L
from shot_vae_amd import calibration as CA
from oracle import smooth_oracle as SO
from tests import _calib_ref as R

SV_E_ARG, SV_E_SHAPE = -1, -2    # include/shotvae_hip.h
PTR = 4096                       # never dereferenced: a refused call launches nothing
TEMP_CASES = [(257, 10, 3.0), (130, 100, 5.0), (65, 2, 2.0)]          # N, K, the scale of the normal logits


# ================================================================================================ against independent sources
def test_detection_counts_reproduce_scikit_learn_on_tied_scores():
    M = pytest.importorskip("sklearn.metrics")
    score, positive = R.detection_case()
    assert positive.sum() == 257 and len(np.unique(score)) < 40, "the case has no ties"
    got = R.detection(score, positive)
    assert got["auroc"] == pytest.approx(M.roc_auc_score(positive, score), abs=1e-12)
    assert got["aupr"] == pytest.approx(M.average_precision_score(positive, score), abs=1e-12)
    assert got["aupr_neg"] == pytest.approx(M.average_precision_score(1 - positive, -score), abs=1e-12)
    for tpr in (0.95, 0.5, 1.0):
        f, t, _ = M.roc_curve(positive, score, drop_intermediate=False)
        assert R.detection(score, positive, tpr)["fpr_at_tpr"] == pytest.approx(f[t >= tpr].min(), abs=1e-12), tpr


def test_aurc_is_the_sorted_cumulative_risk_on_tie_free_data():
    rng = np.random.RandomState(903)
    conf = rng.permutation(300).astype(np.float32) / 300.0
    correct = (rng.uniform(size=300) < 0.3 + 0.6 * conf).astype(np.int64)
    order = np.argsort(-conf)
    risk = np.cumsum(1 - correct[order]) / np.arange(1, 301)
    got = R.selective(conf, correct)
    assert got["aurc"] == pytest.approx(risk.mean(), abs=1e-12)
    # the optimum: the same errors, all ranked last
    best = np.cumsum(np.sort(1 - correct)) / np.arange(1, 301)
    assert got["e_aurc"] == pytest.approx(risk.mean() - best.mean(), abs=1e-12) and got["e_aurc"] > 0
    # a confidence that ranks every error last attains it
    ideal = np.where(correct == 1, 1.0 + conf, conf).astype(np.float32)
    assert R.selective(ideal, correct)["e_aurc"] == pytest.approx(0.0, abs=1e-12)


def test_ece_of_a_hand_counted_three_bin_case():
    # bins (0, 1/3], (1/3, 2/3], (2/3, 1]:   bin 0: 0.25 (hit), 0.3 (miss);   bin 1: empty;   bin 2: 0.7 (hit), 0.9 (hit), 1.0 (miss), 0.75 (hit)
    conf = np.array([0.25, 0.7, 0.9, 0.3, 1.0, 0.75], dtype=np.float32)
    pred = np.array([1, 0, 2, 1, 0, 2])
    label = np.array([1, 0, 2, 0, 1, 2])
    edges = R.uniform_edges(3)
    bc, bk, counts, sums = R.accum(conf, pred, label, None, None, None, 3, edges, 1)
    assert bc.tolist() == [2, 0, 4] and bk.tolist() == [1, 0, 3] and counts.tolist() == [6, 4, 6]
    out, diagram = R.finish(bc, bk, counts, sums)
    c0, c2 = (np.float64(conf[0]) + np.float64(conf[3])) / 2, (np.float64(conf[1]) + conf[2] + conf[4] + conf[5]) / 4
    assert out[2] == pytest.approx(2 / 6 * abs(0.5 - c0) + 4 / 6 * abs(0.75 - c2), abs=1e-15)
    assert out[3] == pytest.approx(max(abs(0.5 - c0), abs(0.75 - c2)), abs=1e-15)
    assert out[0] == 4 / 6 and out[7] == 6 and np.isnan(diagram[:, 1]).all() and diagram[0, 2] == 0.75
    # a confidence exactly on an inner edge belongs to the bin below: (lo, hi]
    third = edges[1]
    assert R.bin_of(np.array([third, np.nextafter(third, np.float32(1)), 0.0, -1.0, 2.0], dtype=np.float32), edges).tolist() == [0, 1, 0, 0, 2]


@pytest.mark.parametrize("N,K,scale", TEMP_CASES)
def test_newton_on_beta_finds_scipys_temperature(N, K, scale):
    opt = pytest.importorskip("scipy.optimize")
    x, label = R.logits(N, K, scale, 905 + K)
    res = opt.minimize_scalar(lambda b: R.total_nll(x, K, label, R.LOGIT, b), bounds=(1e-3, 1e3), method="bounded",
                              options=dict(xatol=1e-12))
    beta = R.newton(x, K, label, iters=8)
    print("FIG newton %s beta %.9f scipy %.9f" % ((N, K), beta, res.x))
    assert abs(beta - res.x) <= 1e-7
    # the sums are the derivatives of the summed NLL
    sums, count = R.temp_sums(x, K, label, R.LOGIT, 0.7, 1)
    b, h = float(np.float32(0.7)), 1e-4
    f = lambda t: R.total_nll(x, K, label, R.LOGIT, t)          # noqa: E731
    assert sums[0, 0] == pytest.approx((f(b + h) - f(b - h)) / (2 * h), rel=1e-6)
    assert sums[0, 1] == pytest.approx((f(b + h) - 2 * f(b) + f(b - h)) / h ** 2, rel=1e-4)
    assert sums[0, 2] == pytest.approx(f(b), rel=1e-12) and count[0] == N and sums[0, 1] > 0
    # the probability form of the same posterior has the same optimum
    prob = R.probabilities(N, K, scale, 905 + K)[0]
    assert abs(R.newton(prob, K, label, kind=R.PROB, iters=8) - res.x) <= 1e-4 * res.x


def test_temp_update_cases():
    one = lambda a, v, beta=2.0: R.temp_update(np.array([[a, v, 3.0]]), np.array([4]), beta)          # noqa: E731
    new, temp, stats = one(1.0, 4.0)
    assert new == 1.75 and temp == np.float32(1 / 1.75) and stats.tolist() == [0.75, 0.25, -0.25, 1.75]
    assert one(100.0, 1.0)[0] == 0.5 and one(-100.0, 1.0)[0] == 8.0                    # both clamps
    assert one(1.0, 0.0)[0] == 2.0 and one(np.nan, 1.0)[0] == 2.0 and one(1.0, np.inf)[0] == 2.0
    assert np.isnan(R.temp_update(np.zeros((2, 3)), np.zeros(2, np.int64), 1.0)[2][:2]).all()


# ================================================================================================ identities
def test_identities():
    x, label = R.logits(65, 10, 3.0, 907)
    hot = R.rows(x, 10, label, T=1e30)
    assert np.abs(hot["conf"] - 0.1).max() < 1e-12 and np.abs(hot["entropy"] - np.log(10)).max() < 1e-12
    # one-hot probabilities with the correct labels
    onehot = np.eye(10, dtype=np.float32)[label]
    r = R.rows(onehot, 10, label, kind=R.PROB)
    assert np.array_equal(r["pred"], label) and (r["conf"] == 1).all() and (r["nll"] == 0).all() and (r["brier"] == 0).all()
    assert (r["entropy"] == 0).all()
    st = R.accum(r["conf"], r["pred"], label, r["nll"], r["brier"], r["entropy"], 10, R.uniform_edges(15), 3)
    out, _ = R.finish(*st)
    assert out[0] == 1 and out[2] == 0 and out[3] == 0 and out[4] == 0 and out[5] == 0
    # the first maximum; rows that are not finite; labels outside the classes
    t = R.rows(np.array([[1, 3, 3, 0], [np.nan, 0, 0, 0], [np.inf, 0, 0, 0], [-np.inf] * 4, [-np.inf, 0, -np.inf, 0]], dtype=np.float32), 4,
               np.array([1, 1, 1, 1, 7]))
    assert t["pred"].tolist() == [1, -1, -1, -1, 1] and np.isnan(t["conf"][1:4]).all() and t["conf"][4] == 0.5
    assert np.isnan(t["nll"][4]) and np.isnan(t["brier"][4]) and t["entropy"][4] == pytest.approx(np.log(2))
    # a perfect detector, and one that cannot tell anything
    score = np.concatenate([np.linspace(1, 2, 20), np.linspace(-1, 0, 30)]).astype(np.float32)
    positive = np.concatenate([np.ones(20), np.zeros(30)])
    d = R.detection(score, positive)
    assert d == dict(auroc=1.0, aupr=1.0, aupr_neg=1.0, fpr_at_tpr=0.0)
    assert R.detection(np.full(50, 0.25, dtype=np.float32), positive)["auroc"] == 0.5
    # NaN scores are left out; -0 == 0
    withnan = np.concatenate([score, [np.nan, np.nan]]).astype(np.float32)
    assert R.detection(withnan, np.concatenate([positive, [1, 0]])) == d
    gt, eq = R.rank_counts(np.array([0.0, np.nan, np.inf], np.float32), np.array([-0.0, 0.0, np.nan, np.inf, -np.inf, 1.0], np.float32))
    assert gt.tolist() == [2, 0, 0] and eq.tolist() == [2, 0, 1]


def test_the_reference_decides_every_prediction_of_the_large_case():
    """normal logits of scale 3 at (4097, 10): no row's two largest values are closer than twice the fp32 allowance"""
    x, label = R.logits(4097, 10, 3.0, 7201)
    ref, tol = R.row_allowance(x, 10, label, R.LOGIT, 1.0)
    assert (ref["gap"] > 2.0 * max(tol.values())).all()


# ================================================================================================ the C ABI without a GPU
def _rows(**kw):
    a = dict(kind=0, x=PTR, ldx=16, N=5, K=10, temp=None, label=None, pred=PTR, conf=PTR, nll=PTR, brier=PTR, entropy=PTR)
    a.update(kw)
    return L.lib().sv_calib_rows(a["kind"], a["x"], a["ldx"], a["N"], a["K"], a["temp"], a["label"], a["pred"], a["conf"], a["nll"],
                                 a["brier"], a["entropy"], None)


def _accum(**kw):
    a = dict(conf=PTR, pred=PTR, label=PTR, nll=None, brier=None, entropy=None, N=5, K=10, edges=PTR, B=15, bin_count=PTR, bin_correct=PTR,
             counts=PTR, sums=PTR, P=2, init=1)
    a.update(kw)
    return L.lib().sv_calib_accum(a["conf"], a["pred"], a["label"], a["nll"], a["brier"], a["entropy"], a["N"], a["K"], a["edges"], a["B"],
                                  a["bin_count"], a["bin_correct"], a["counts"], a["sums"], a["P"], a["init"], None)


def _finish(**kw):
    a = dict(bin_count=PTR, bin_correct=PTR, counts=PTR, sums=PTR, P=2, B=15, out=PTR, diagram=None)
    a.update(kw)
    return L.lib().sv_calib_finish(a["bin_count"], a["bin_correct"], a["counts"], a["sums"], a["P"], a["B"], a["out"], a["diagram"], None)


def _taccum(**kw):
    a = dict(kind=1, x=PTR, ldx=10, N=5, K=10, label=PTR, beta=PTR, sums=PTR, count=PTR, P=2, init=1)
    a.update(kw)
    return L.lib().sv_temp_accum(a["kind"], a["x"], a["ldx"], a["N"], a["K"], a["label"], a["beta"], a["sums"], a["count"], a["P"],
                                 a["init"], None)


def _tupdate(**kw):
    a = dict(sums=PTR, count=PTR, P=2, beta=PTR, temp=PTR, stats=PTR)
    a.update(kw)
    return L.lib().sv_temp_update(a["sums"], a["count"], a["P"], a["beta"], a["temp"], a["stats"], None)


def _scan(**kw):
    a = dict(q=PTR, Q=5, g=PTR, g_w=None, N=7, P=2, greater=PTR, equal=PTR)
    a.update(kw)
    return L.lib().sv_rank_scan(a["q"], a["Q"], a["g"], a["g_w"], a["N"], a["P"], a["greater"], a["equal"], None)


SIZES = (0, -3)
BAD_P = [(dict(P=v), SV_E_SHAPE, b"P=%d" % v) for v in (0, 65, -1)]
BAD_B = [(dict(B=v), SV_E_SHAPE, b"B=%d" % v) for v in (0, 1025, -2)]


@pytest.mark.parametrize("fn,name,cases", [
    (_rows, b"sv_calib_rows",
     [(dict(x=None), SV_E_ARG, b"NULL"), (dict(pred=None, conf=None, nll=None, brier=None, entropy=None), SV_E_ARG, b"NULL"),
      (dict(kind=2), SV_E_ARG, b"kind"), (dict(kind=-1), SV_E_ARG, b"kind"), (dict(ldx=9), SV_E_SHAPE, b"ldx=9")]
     + [(dict([(k, v)]), SV_E_ARG, b"size") for k in ("N", "K") for v in SIZES]),
    (_accum, b"sv_calib_accum",
     [(dict([(k, None)]), SV_E_ARG, b"NULL") for k in ("conf", "pred", "label", "edges", "bin_count", "bin_correct", "counts", "sums")]
     + [(dict([(k, v)]), SV_E_ARG, b"size") for k in ("N", "K") for v in SIZES] + BAD_B + BAD_P),
    (_finish, b"sv_calib_finish",
     [(dict([(k, None)]), SV_E_ARG, b"NULL") for k in ("bin_count", "bin_correct", "counts", "sums", "out")] + BAD_B + BAD_P),
    (_taccum, b"sv_temp_accum",
     [(dict([(k, None)]), SV_E_ARG, b"NULL") for k in ("x", "label", "beta", "sums", "count")]
     + [(dict(kind=2), SV_E_ARG, b"kind"), (dict(ldx=9), SV_E_SHAPE, b"ldx=9")]
     + [(dict([(k, v)]), SV_E_ARG, b"size") for k in ("N", "K") for v in SIZES] + BAD_P),
    (_tupdate, b"sv_temp_update",
     [(dict([(k, None)]), SV_E_ARG, b"NULL") for k in ("sums", "count", "beta", "temp", "stats")] + BAD_P),
    (_scan, b"sv_rank_scan",
     [(dict([(k, None)]), SV_E_ARG, b"NULL") for k in ("q", "g", "greater", "equal")]
     + [(dict([(k, v)]), SV_E_ARG, b"size") for k in ("Q", "N") for v in SIZES] + BAD_P),
])
def test_entry_points_refuse_bad_arguments_before_any_launch(fn, name, cases):
    for kw, code, word in cases:
        assert fn(**kw) == code, (name, kw)
        err = L.lib().sv_last_error()
        assert word in err and name in err, (kw, err)


def test_entry_points_are_bound_and_exported():
    for name in ("sv_calib_rows", "sv_calib_accum", "sv_calib_finish", "sv_temp_accum", "sv_temp_update", "sv_rank_scan"):
        assert name in L.EXPORTS and hasattr(L.lib(), name)
    assert L.lib().sv_version() == L.ABI_VERSION == 8
    for name in ("row_stats", "Reliability", "TemperatureScaler", "rank_counts", "detection_metrics", "selective_metrics",
                 "evaluate_calibration", "evaluate_detection"):
        assert getattr(S, name) is getattr(CA, name)


# ================================================================================================ the Python layer
def test_python_layer_refuses_cpu_tensors_and_bad_arguments():
    x, y, flag = torch.zeros(6, 10), torch.zeros(6, dtype=torch.int64), torch.zeros(10, dtype=torch.int64)
    for call in (lambda: S.row_stats(x, y), lambda: S.Reliability(10).update(x, y), lambda: S.TemperatureScaler().step(x, y),
                 lambda: S.TemperatureScaler().fit(x, y), lambda: S.rank_counts(x[0], x[1]), lambda: S.detection_metrics(x[0], flag),
                 lambda: S.selective_metrics(x[0], flag)):
        with pytest.raises(L.ShotVaeHipError, match="MI355X"):
            call()
    with pytest.raises(ValueError, match="unknown kind"):
        S.row_stats(x, y, kind="softmax")
    with pytest.raises(ValueError, match="unknown kind"):
        S.TemperatureScaler("softmax")
    for bad in (x.view(-1), torch.zeros(0, 10)):
        with pytest.raises(ValueError, match="matrix"):
            S.row_stats(bad)
    with pytest.raises(ValueError, match="integer vector"):
        S.row_stats(x, y[:5])
    with pytest.raises(ValueError, match="temperature must be"):
        S.row_stats(x, y, temperature=0.0)
    with pytest.raises(ValueError, match="temperature must be"):
        S.row_stats(x, y, temperature=torch.ones(2))
    for bins in (0, 1025):
        with pytest.raises(ValueError, match="bins must be"):
            S.Reliability(10, bins=bins)
    with pytest.raises(ValueError, match="non-decreasing"):
        S.Reliability(10, edges=[0.0, 0.6, 0.5, 1.0])
    with pytest.raises(ValueError, match="num_classes"):
        S.Reliability(0)
    rel = S.Reliability(10, edges=[0.0, 0.5, 1.0])
    assert rel.bins == 2 and len(rel) == 0
    with pytest.raises(ValueError, match="10 classes"):
        rel.update(torch.zeros(6, 9), y)
    with pytest.raises(ValueError, match="labels are required"):
        rel.update(x, None)
    with pytest.raises(ValueError, match="no rows"):
        rel.result()
    with pytest.raises(ValueError, match="iters"):
        S.TemperatureScaler().fit(x, y, iters=0)
    with pytest.raises(ValueError, match="tpr"):
        S.detection_metrics(x[0], flag, tpr=0.0)
    with pytest.raises(ValueError, match="vector"):
        S.detection_metrics(x[0], y)


def test_evaluators_check_their_arguments_before_anything_runs():
    x, y = torch.zeros(2, 3, 32, 32), torch.zeros(2, dtype=torch.int64)
    vae = S.VariationalAutoEncoder("wideresnet-10-1", num_input_channels=3, img_size=(32, 32), data_parallel=False,
                                   continuous_latent_dim=128, disc_latent_dim=10, small_input=True, compute_dtype="fp32")
    smooth = S.SmoothVAE((SO.KINDS["svhn"]["in_ch"], 32, 32), {"cont": 32, "disc": [10]}, compute_dtype="fp32")
    clf = S.WideResNetClassifier(num_input_channels=3, depth=10, width=1, num_classes=10, data_parallel=False, compute_dtype="fp32")
    crit = S.VAECriterion(discrete_dim=10, x_sigma=1.0, bce_reconstruction=True)
    for m in (smooth, clf):
        m.eval()
        for score in ("elbo", "log_px"):
            with pytest.raises(ValueError, match="needs a decoder"):
                S.evaluate_detection(m, [x], [x], score=score, criterion=crit)
    for m in (vae, smooth, clf):
        m.train()
        with pytest.raises(NotImplementedError, match="eval mode only"):
            S.evaluate_calibration(m, [(x, y)])
        with pytest.raises(NotImplementedError, match="eval mode only"):
            S.evaluate_detection(m, [x], [x])
        m.eval()
        with pytest.raises(L.ShotVaeHipError, match="MI355X"):
            S.evaluate_calibration(m, [(x, y)])
        with pytest.raises(L.ShotVaeHipError, match="MI355X"):
            S.evaluate_detection(m, [x], [x])
        with pytest.raises(ValueError, match="empty"):
            S.evaluate_calibration(m, [])
        with pytest.raises(ValueError, match=r"\(image, label\)"):
            S.evaluate_calibration(m, [x])
        with pytest.raises(ValueError, match="score must be"):
            S.evaluate_detection(m, [x], [x], score="energy")
        with pytest.raises(ValueError, match="takes no criterion"):
            S.evaluate_detection(m, [x], [x], score="msp", criterion=crit)
        assert not m.training
    with pytest.raises(ValueError, match="needs the criterion"):
        S.evaluate_detection(vae, [x], [x], score="elbo")
    for fn in (lambda m: S.evaluate_calibration(m, [(x, y)]), lambda m: S.evaluate_detection(m, [x], [x])):
        with pytest.raises(TypeError, match="WideResNetClassifier"):
            fn(torch.nn.Linear(2, 2))
