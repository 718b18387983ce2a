"""Calibration, temperature scaling and rank counts on a real MI355X: sv_calib_rows, sv_calib_accum, sv_calib_finish, sv_temp_accum,
sv_temp_update and sv_rank_scan through the C ABI against the restatement of tests/_calib_ref.py (pinned to scikit-learn, scipy and
hand-counted cases by tests/test_calib_cpu.py), then the Python layer (shot_vae_amd.calibration).

Integer results and double sums are compared exactly (the restatement adds in the kernels' order).  Otherwise the allowances follow the
project's 8x rule and are measured when the test runs, never taken from a GPU result: 8 x the error of the fp32 numpy restatement
against float64 on the case's own inputs -- for a per-row value the largest error over the case's rows (R.row_allowance), for a sum of
per-row values the sum of the rows' errors (each row may be 8 x as far as the restatement's, and so may their sum).  A prediction is
compared with float64 only on the rows whose two largest z are further apart than twice the largest allowance of the case; the share
of rows left out is asserted (on the CPU side) to stay under 1 %.  Outputs are pre-filled and carry guard rows.

Measured on an MI355X, error (allowance): sv_calib_rows over the eight shapes, both kinds and T = none / 1 / 0.5 / 3: conf up to 2.9e-7,
nll 5.1e-6, brier 3.9e-7, entropy 1.0e-6, at most 0.38 / 0.29 / 0.19 / 0.25 of the case's allowance (8.8e-8 .. 3.0e-5; 0 at K = 1, where
the results are exact), no prediction undecided in any case; the temperature sums a 2.8e-5 (1.2e-3), v 2.4e-4 (2.1e-3), nll 8.7e-5
(5.2e-4) at the most, under 0.2 of the allowance everywhere; twelve Newton iterations against scipy's T: 1.0e-7 (9.5e-7) at (257, 10),
4.7e-8 (1.9e-6) at (130, 100), 1.7e-8 (1.9e-6) at (65, 2); the other comparisons are equalities or 1-ulp bounds."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import shot_vae_amd as S                                        # noqa: E402
from shot_vae_amd import _lib as L                              # noqa: E402
from oracle import closed_form as CF                            # noqa: E402
from tests import _calib_ref as R                               # noqa: E402
from tests import _classifier_oracle as Q                       # noqa: E402
from tests import _knn_ref as KR                                # noqa: E402

GUARD = 3
FILL = -7.0


def dev():
    return torch.device("cuda:0")


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev())


def f64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev())


def i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev())


def ulp32(a):
    return np.spacing(np.abs(np.asarray(a, dtype=np.float32))).astype(np.float64)


def same(a, b):
    """equal, NaN in the same places"""
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def padded(x, ldx):
    """x [N, K] in a matrix of row stride ldx whose pad columns hold NaN"""
    out = np.full((x.shape[0], ldx), np.nan, dtype=np.float32)
    out[:, :x.shape[1]] = x
    return out


# ================================================================================================ sv_calib_rows
FIELDS = ("pred", "conf", "nll", "brier", "entropy")


def calib_rows(x, K, ldx, kind, T=None, label=None, want=FIELDS):
    """sv_calib_rows on padded(x) -> dict of numpy arrays [N] for the outputs in `want`; the others, and the guard rows, stay as they
    were.  T: None (temp == NULL) or a number (a device float)."""
    N = x.shape[0]
    dx = f32(padded(x[:, :K], ldx))
    out = {f: torch.full((N + GUARD,), int(FILL) if f == "pred" else FILL, dtype=torch.int64 if f == "pred" else torch.float32,
                         device=dev()) for f in FIELDS}
    temp = None if T is None else f32(np.array([T]))
    lab = None if label is None else i64(label)
    L.call("sv_calib_rows", kind, p(dx), ldx, N, K, p(temp), p(lab), *[p(out[f]) if f in want else None for f in FIELDS], st())
    torch.cuda.synchronize()
    for f in FIELDS:
        t = out[f].cpu().numpy()
        assert (t[N:] == FILL).all(), "sv_calib_rows wrote behind %s" % f
        assert f in want or (t == FILL).all(), "sv_calib_rows wrote %s, which was not asked for" % f
    return {f: out[f][:N].cpu().numpy() for f in want}


# (257, 300, 304): beyond 4 x 64 classes a row is read again by every pass
ROW_SHAPES = [(1, 1, 1), (65, 2, 2), (130, 10, 16), (63, 130, 136), (257, 65, 65), (130, 100, 104), (4097, 10, 10), (257, 300, 304)]


@pytest.mark.parametrize("kind", [R.LOGIT, R.PROB])
@pytest.mark.parametrize("N,K,ldx", ROW_SHAPES)
def test_rows_match_float64(N, K, ldx, kind):
    x, label = (R.logits if kind == R.LOGIT else R.probabilities)(N, K, 3.0, 7200 + K)
    for T in (None, 1.0, 0.5, 3.0):
        ref, tol = R.row_allowance(x, K, label, kind, 1.0 if T is None else T)
        decided = ref["gap"] > 2.0 * max(tol.values())
        assert (~decided).sum() <= N // 100, "the reference alone leaves more than 1 % of the rows undecided"
        got = calib_rows(x, K, ldx, kind, T, label)
        assert np.array_equal(got["pred"][decided], ref["pred"][decided])
        assert (got["pred"] >= 0).all() and (got["pred"] < K).all()
        for f in R.ROW_FIELDS:
            err = float(np.abs(got[f].astype(np.float64) - ref[f]).max())
            print("FIG rows %s kind %d T %s %s err %.3e tol %.3e undecided %d" % ((N, K, ldx), kind, T, f, err, tol[f], int((~decided).sum())))
            assert err <= tol[f], (f, T)


def test_the_large_logit_case_leaves_no_prediction_out():
    x, label = R.logits(4097, 10, 3.0, 7200 + 10)
    ref, tol = R.row_allowance(x, 10, label, R.LOGIT, 1.0)
    assert (ref["gap"] > 2.0 * max(tol.values())).all()
    assert np.array_equal(calib_rows(x, 10, 10, R.LOGIT, None, label)["pred"], ref["pred"])


@pytest.mark.parametrize("N,K,ldx", [(65, 2, 2), (130, 10, 16), (257, 65, 65), (63, 130, 136), (65, 300, 304)])
def test_rows_take_the_first_maximum_on_exact_ties(N, K, ldx):
    x = np.floor(CF.uniform((N, K), 7301, 0.0, 3.0).numpy().astype(np.float64)).astype(np.float32)          # 0, 1, 2: ties abound
    ref = R.rows(x, K)
    assert ((x == x.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum() >= N // 4, "the case has no ties"
    for kind, data, T in ((R.LOGIT, x, None), (R.LOGIT, x, 0.5), (R.PROB, x + 1.0, 2.0)):
        assert np.array_equal(calib_rows(data, K, ldx, kind, T, want=("pred",))["pred"], ref["pred"]), (kind, T)


def test_rows_that_are_not_finite_and_labels_outside_the_classes():
    N, K = 70, 10
    x, label = R.logits(N, K, 3.0, 7303)
    x[3, 5] = np.nan
    x[65, 0] = np.inf
    x[66, :] = -np.inf
    x[67, :9] = -np.inf                                    # one finite class: p = 1 there
    x[68, 2] = -np.inf                                     # a class of probability 0
    label[67], label[68] = 9, 2                            # ... the label of row 68: nll = +inf
    label[10], label[11], label[12] = -1, K, 2 ** 40
    ref, tol = R.row_allowance(x, K, label, R.LOGIT, 1.0)
    got = calib_rows(x, K, 16, R.LOGIT, None, label)
    bad, foreign = [3, 65, 66], [10, 11, 12]
    assert (got["pred"][bad] == -1).all() and all(np.isnan(got[f][bad]).all() for f in R.ROW_FIELDS)
    assert np.isnan(got["nll"][foreign]).all() and np.isnan(got["brier"][foreign]).all() and np.isfinite(got["conf"][foreign]).all()
    assert got["pred"][67] == 9 and got["conf"][67] == 1 and got["nll"][67] == 0 and got["brier"][67] == 0 and got["entropy"][67] == 0
    assert np.isposinf(got["nll"][68]) and np.isposinf(ref["nll"][68])
    assert same(got["pred"], ref["pred"])
    for f in R.ROW_FIELDS:
        assert np.array_equal(np.isnan(got[f]), np.isnan(ref[f])), f
        ok = np.isfinite(ref[f])
        assert np.abs(got[f][ok] - ref[f][ok]).max() <= tol[f], f
    none = calib_rows(x, K, 16, R.LOGIT, None, None)                   # label == NULL
    assert np.isnan(none["nll"]).all() and np.isnan(none["brier"]).all() and same(none["conf"], got["conf"])
    # a temperature that is not > 0: every row NaN
    for T in (0.0, -1.0, np.nan):
        assert (calib_rows(x, K, 16, R.LOGIT, T, label)["pred"] == -1).all()
    # probabilities: zeros are classes of probability 0, a negative entry makes the row NaN
    q, qlabel = R.probabilities(N, K, 3.0, 7305)
    q[5, :] = 0.0
    q[6, :] = 0.0
    q[6, 4] = 0.25                                         # not normalised: p = 1 at class 4
    q[7, 1] = -0.5
    q[8, 3] = 0.0
    qlabel[8] = 3
    ref, tol = R.row_allowance(q, K, qlabel, R.PROB, 2.0)
    got = calib_rows(q, K, 10, R.PROB, 2.0, qlabel)
    assert got["pred"][[5, 7]].tolist() == [-1, -1] and got["pred"][6] == 4 and got["conf"][6] == 1 and np.isposinf(got["nll"][8])
    assert same(got["pred"], ref["pred"])
    for f in R.ROW_FIELDS:
        ok = np.isfinite(ref[f])
        assert np.array_equal(np.isnan(got[f]), np.isnan(ref[f])) and np.abs(got[f][ok] - ref[f][ok]).max() <= tol[f], f


def test_every_subset_of_the_outputs_leaves_the_others_untouched():
    x, label = R.logits(65, 10, 3.0, 7307)
    full = calib_rows(x, 10, 16, R.LOGIT, 0.5, label)
    for r in range(1, len(FIELDS)):
        for want in itertools.combinations(FIELDS, r):
            got = calib_rows(x, 10, 16, R.LOGIT, 0.5, label, want=want)          # (checks the outputs not asked for)
            assert all(same(got[f], full[f]) for f in want), want


# ================================================================================================ sv_calib_accum / sv_calib_finish
def accum_case(N, K, B, seed):
    """per-row values made in numpy: confidences on an inner edge, below edges[0] and above edges[B]; pred = -1; foreign labels"""
    rng = np.random.RandomState(seed)
    edges = R.uniform_edges(B)
    conf = rng.uniform(size=N).astype(np.float32)
    pred = rng.randint(0, K, size=N).astype(np.int64)
    label = np.where(rng.uniform(size=N) < 0.6, pred, rng.randint(0, K, size=N)).astype(np.int64)
    for j, i in enumerate(range(0, N, 7)):
        conf[i] = (edges[1 + j % (B - 1)] if B > 1 else 0.5, -0.5, 1.5, 0.0, 1.0)[j % 5]
    if N > 8:
        pred[2], label[4], label[5], label[6] = -1, -1, K, 2 ** 40
    nll, brier, entropy = (rng.uniform(0.0, 3.0, size=N).astype(np.float32) for _ in range(3))
    return conf, pred, label, nll, brier, entropy, edges


class AccumState:
    """the device side of a sequence of sv_calib_accum calls: zeroed integers, garbage in the sums, guards behind everything"""

    def __init__(self, B, P, fill=7.0):
        self.B, self.P, self.fill = B, P, fill
        self.ints = torch.zeros(2 * B + 3 + GUARD, dtype=torch.int64, device=dev())
        self.ints[2 * B + 3:] = -7
        self.sums = torch.full((P * (B + 3) + GUARD,), fill, dtype=torch.float64, device=dev())

    def call(self, K, edges, conf, pred, label, nll, brier, entropy, lo, hi, init):
        B = self.B
        L.call("sv_calib_accum", p(conf[lo:]), p(pred[lo:]), p(label[lo:]), p(nll[lo:]) if nll is not None else None,
               p(brier[lo:]) if brier is not None else None, p(entropy[lo:]) if entropy is not None else None, hi - lo, K, p(edges), B,
               p(self.ints[:B]), p(self.ints[B:]), p(self.ints[2 * B:]), p(self.sums), self.P, init, st())

    def read(self):
        torch.cuda.synchronize()
        B, P = self.B, self.P
        ints, sums = self.ints.cpu().numpy(), self.sums.cpu().numpy()
        assert (ints[2 * B + 3:] == -7).all() and (sums[P * (B + 3):] == self.fill).all(), "sv_calib_accum wrote behind its states"
        return ints[:B], ints[B:2 * B], ints[2 * B:2 * B + 3], sums[:P * (B + 3)].reshape(P, B + 3)


def run_accum(case, K, P, cuts=None, **kw):
    conf, pred, label, nll, brier, entropy, edges = case
    state = AccumState(len(edges) - 1, P, **kw)
    d = [f32(conf), i64(pred), i64(label), f32(nll), f32(brier), f32(entropy)]
    marks = [0] + list(cuts or []) + [len(conf)]
    for n, (lo, hi) in enumerate(zip(marks[:-1], marks[1:])):
        state.call(K, f32(edges), *d, lo, hi, 1 if n == 0 else 0)
    return state.read()


def states_equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("B", [1, 15, 64, 65, 1024])
@pytest.mark.parametrize("N", [1, 63, 65, 130, 4097])
def test_accum_counts_exactly_and_sums_in_the_restatements_order(N, B):
    K = 10
    case = accum_case(N, K, B, 7400 + N + B)
    for P in (1, 3, 64):
        want = R.accum(*case[:6], K, case[6], P)
        got = run_accum(case, K, P)
        assert states_equal(got[:3], want[:3]), P
        assert np.array_equal(got[3], want[3]), "the sums of a state are not the sequential double sums (P = %d)" % P
    if N > 8:
        b = R.bin_of(case[0], case[6])
        assert want[2][0] == N - 4 and b.min() == 0 and b.max() == B - 1


def test_accum_cut_rules_init_flag_accumulation_and_repeats():
    N, K, B = 4097, 10, 15
    case = accum_case(N, K, B, 7411)
    for P, cuts in ((1, [64, 1984]), (1, list(range(640, 4097, 640))), (3, [192, 1920]), (64, [4096])):
        one = run_accum(case, K, P)
        assert states_equal(one, run_accum(case, K, P)), "a repeat differs"
        assert states_equal(one, run_accum(case, K, P, cuts=cuts, fill=-3.0)), (P, cuts)
        assert states_equal(one, R.accum(*case[:6], K, case[6], P))
    # init = 0 continues the states and the integers accumulate: the same rows twice
    conf, pred, label, nll, brier, entropy, edges = case
    state = AccumState(B, 3)
    d = [f32(conf), i64(pred), i64(label), f32(nll), f32(brier), f32(entropy)]
    state.call(K, f32(edges), *d, 0, N, 1)
    state.call(K, f32(edges), *d, 0, N, 0)
    first = R.accum(*case[:6], K, edges, 3)
    assert states_equal(state.read(), R.accum(*case[:6], K, edges, 3, state=first))
    # a NULL input array leaves its total untouched (init = 0), and zero after init = 1
    state = AccumState(B, 3, fill=5.0)
    state.call(K, f32(edges), d[0], d[1], d[2], None, d[4], None, 0, N, 0)
    sums = state.read()[3]
    assert (sums[:, B] == 5.0).all() and (sums[:, B + 2] == 5.0).all() and (sums[:, B + 1] != 5.0).all()
    state = AccumState(B, 3, fill=5.0)
    state.call(K, f32(edges), d[0], d[1], d[2], None, d[4], None, 0, N, 1)
    assert states_equal(state.read(), R.accum(conf, pred, label, None, brier, None, K, edges, 3))


def finish(bc, bk, counts, sums, want_diagram=True):
    P, B = sums.shape[0], len(bc)
    out = torch.full((8 + GUARD,), FILL, dtype=torch.float32, device=dev())
    diagram = torch.full((2 * B + GUARD,), FILL, dtype=torch.float32, device=dev())
    dbc, dbk, dcounts, dsums = i64(bc), i64(bk), i64(counts), f64(sums)
    L.call("sv_calib_finish", p(dbc), p(dbk), p(dcounts), p(dsums), P, B, p(out), p(diagram) if want_diagram else None, st())
    torch.cuda.synchronize()
    out, diagram = out.cpu().numpy(), diagram.cpu().numpy()
    assert (out[8:] == FILL).all() and (diagram[2 * B:] == FILL).all() and (want_diagram or (diagram == FILL).all())
    return out[:8], diagram[:2 * B].reshape(2, B)


def within_one_ulp(got, ref):
    near = ref.astype(np.float32)
    return np.array_equal(np.isnan(got), np.isnan(ref)) and (np.nan_to_num(np.abs(got.astype(np.float64) - near)) <= np.nan_to_num(ulp32(near))).all()


@pytest.mark.parametrize("N,B,P", [(4097, 15, 3), (130, 65, 64), (63, 1024, 1), (4097, 1, 1), (1, 15, 64)])
def test_finish_rounds_the_float64_restatement_once(N, B, P):
    state = R.accum(*accum_case(N, 10, B, 7421)[:6], 10, R.uniform_edges(B), P)
    ref_out, ref_diagram = R.finish(*state)
    out, diagram = finish(*state)
    assert within_one_ulp(out, ref_out) and within_one_ulp(diagram, ref_diagram)
    assert B < 15 or N > 1000 or np.isnan(diagram).any(), "the case has no empty bin"
    assert same(finish(*state, want_diagram=False)[0], out)


def test_finish_without_a_valid_row():
    B, P = 15, 3
    out, diagram = finish(np.zeros(B, np.int64), np.zeros(B, np.int64), np.array([0, 0, 40]), np.zeros((P, B + 3)))
    assert np.isnan(out[:7]).all() and out[7] == 0 and np.isnan(diagram).all()


# ================================================================================================ sv_temp_accum / sv_temp_update
TEMP_CASES = [(257, 10, 3.0), (130, 100, 5.0), (65, 2, 2.0)]          # the shapes tests/test_calib_cpu.py checks against scipy


def temp_accum(x, K, ldx, label, kind, beta, P, cuts=None):
    N = x.shape[0]
    dx, dl, db = f32(padded(x, ldx)), i64(label), f64(np.array([beta]))
    sums = torch.full((3 * P + GUARD,), 7.0, dtype=torch.float64, device=dev())
    count = torch.full((P + GUARD,), -7, dtype=torch.int64, device=dev())
    marks = [0] + list(cuts or []) + [N]
    for n, (lo, hi) in enumerate(zip(marks[:-1], marks[1:])):
        L.call("sv_temp_accum", kind, p(dx[lo:]), ldx, hi - lo, K, p(dl[lo:]), p(db), p(sums), p(count), P, 1 if n == 0 else 0, st())
    torch.cuda.synchronize()
    assert bool((sums[3 * P:] == 7.0).all()) and bool((count[P:] == -7).all()), "sv_temp_accum wrote behind its states"
    return sums[:3 * P].view(P, 3).cpu().numpy(), count[:P].cpu().numpy()


@pytest.mark.parametrize("kind", [R.LOGIT, R.PROB])
@pytest.mark.parametrize("N,K,scale", TEMP_CASES)
def test_temp_sums_match_float64(N, K, scale, kind):
    x, label = (R.logits if kind == R.LOGIT else R.probabilities)(N, K, scale, 905 + K)
    label = label.copy()
    if N > 8:
        label[3], label[5] = -1, K                         # foreign labels: not rows of the sum
    for beta in (0.25, 1.0, 4.0):
        ref = R.temp_terms(x, K, label, kind, beta)
        low = R.temp_terms(x, K, label, kind, beta, dtype=np.float32)
        valid = ref[3]
        assert np.array_equal(valid, low[3]) and valid.sum() == (N - 2 if N > 8 else N)
        for P in (1, 3):
            sums, count = temp_accum(x, K, K + (6 if K == 10 else 0), label, kind, beta, P)
            assert count.sum() == valid.sum() and np.array_equal(count, R.temp_sums(x, K, label, kind, beta, P)[1])
            for j, name in enumerate(("a", "v", "nll")):
                want = float(ref[j][valid].sum())
                tol = 8.0 * float(np.abs(low[j][valid].astype(np.float64) - ref[j][valid]).sum())
                err = abs(float(sums[:, j].sum()) - want)
                print("FIG temp %s kind %d beta %g P %d %s err %.3e tol %.3e" % ((N, K), kind, beta, P, name, err, tol))
                assert err <= tol, (name, beta, P)
        again = temp_accum(x, K, K + (6 if K == 10 else 0), label, kind, beta, 3)
        assert np.array_equal(again[0], sums) and np.array_equal(again[1], count), "a repeat differs"
    # cut at a multiple of 64 P: the states hold the bits of the one call
    if N > 192:
        assert np.array_equal(temp_accum(x, K, K, label, kind, 1.0, 3, cuts=[192])[0], temp_accum(x, K, K, label, kind, 1.0, 3)[0])
        assert np.array_equal(temp_accum(x, K, K, label, kind, 1.0, 1, cuts=[64, 128])[0], temp_accum(x, K, K, label, kind, 1.0, 1)[0])


def temp_update(sums, count, beta):
    P = len(count)
    db, ds, dc = f64(np.array([beta, 7.0])), f64(sums), i64(count)
    temp = torch.full((1 + GUARD,), FILL, dtype=torch.float32, device=dev())
    stats = torch.full((4 + GUARD,), FILL, dtype=torch.float32, device=dev())
    L.call("sv_temp_update", p(ds), p(dc), P, p(db), p(temp), p(stats), st())
    torch.cuda.synchronize()
    assert float(db[1]) == 7.0 and bool((temp[1:] == FILL).all()) and bool((stats[4:] == FILL).all())
    return float(db[0]), temp[:1].cpu().numpy()[0], stats[:4].cpu().numpy()


def test_temp_update_newton_step_both_clamps_and_no_curvature():
    cases = [(np.array([[1.0, 4.0, 3.0], [0.5, 1.0, 2.0], [-0.25, 0.5, 1.0]]), np.array([4, 3, 2]), 2.0),           # a Newton step
             (np.array([[100.0, 1.0, 3.0]]), np.array([4]), 2.0), (np.array([[-100.0, 1.0, 3.0]]), np.array([4]), 2.0),      # the clamps
             (np.array([[1.0, 0.0, 3.0]]), np.array([4]), 2.0), (np.array([[np.nan, 1.0, 3.0]]), np.array([4]), 0.5),        # unchanged
             (np.zeros((2, 3)), np.zeros(2, np.int64), 1.0)]                                                             # no valid row
    moved = []
    for sums, count, beta in cases:
        want, want_temp, want_stats = R.temp_update(sums, count, beta)
        got, temp, stats = temp_update(sums, count, beta)
        assert abs(got - want) <= 4.0 * np.spacing(want) and temp == np.float32(1.0 / got) and temp == want_temp
        assert within_one_ulp(stats, want_stats), (sums.tolist(), stats, want_stats)
        moved.append(got / beta)
    assert 0.25 < moved[0] < 1.0 and moved[1:5] == [0.25, 4.0, 1.0, 1.0] and moved[5] == 1.0


@pytest.mark.parametrize("N,K,scale", TEMP_CASES)
def test_twelve_iterations_find_scipys_temperature(N, K, scale):
    x, label = R.logits(N, K, scale, 905 + K)
    try:
        from scipy.optimize import minimize_scalar
        fixed = minimize_scalar(lambda b: R.total_nll(x, K, label, R.LOGIT, b), bounds=(1e-3, 1e3), method="bounded",
                                options=dict(xatol=1e-12)).x
    except ImportError:                                    # the float64 iteration, which test_calib_cpu.py pins to scipy
        fixed = R.newton(x, K, label, iters=12)
    T = 1.0 / fixed
    low = 1.0 / R.newton(x, K, label, iters=12, dtype=np.float32, P=S.calibration.partials(1, N))
    tol = max(8.0 * abs(low - T), 8.0 * float(ulp32(T)))
    ts = S.TemperatureScaler().fit(f32(x), i64(label), iters=12)
    got = float(ts.temperature.cpu()[0])
    print("FIG fit %s T %.9f scipy %.9f err %.3e tol %.3e last step %.3e" % ((N, K), got, T, abs(got - T), tol, ts.last_step))
    assert abs(got - T) <= tol
    assert ts.temperature.cpu().numpy()[0] == np.float32(1.0 / float(ts.beta.cpu()[0])), "temp is not (float)(1 / beta)"
    assert abs(ts.nll - R.total_nll(x, K, label, R.LOGIT, fixed) / N) <= 1e-5 * max(1.0, abs(ts.nll))
    # the probability form of the same posterior
    prob = R.probabilities(N, K, scale, 905 + K)[0]
    tp = S.TemperatureScaler("prob").fit(f32(prob), i64(label), iters=12)
    assert abs(float(tp.temperature.cpu()[0]) - T) <= 1e-3 * T


# ================================================================================================ sv_rank_scan
def rank_scan(q, g, w, P, cuts=None, into=None):
    Q, N = len(q), len(g)
    dq, dg, dw = f32(q), f32(g), None if w is None else i64(w)
    out = into if into is not None else torch.zeros(2, Q + GUARD, dtype=torch.int64, device=dev())
    marks = [0] + list(cuts or []) + [N]
    for lo, hi in zip(marks[:-1], marks[1:]):
        L.call("sv_rank_scan", p(dq), Q, p(dg[lo:]), p(dw[lo:]) if dw is not None else None, hi - lo, P, p(out[0]), p(out[1]), st())
    torch.cuda.synchronize()
    assert bool((out[:, Q:] == 0).all()), "sv_rank_scan wrote behind its outputs"
    return out[0, :Q].cpu().numpy(), out[1, :Q].cpu().numpy()


@pytest.mark.parametrize("Q,N", [(1, 1), (65, 63), (130, 4097), (4097, 130)])
def test_rank_counts_are_exact_and_independent_of_the_grid(Q, N):
    q, g = R.quarters(Q, 7501), R.quarters(N, 7503)
    w = np.random.RandomState(7505).randint(0, 4, size=N).astype(np.int64)
    if N > 8:
        w[3] = 2 ** 40                                     # beyond 32 bits: the int64 path
    for weights in (None, w):
        want = R.rank_counts(q, g, weights)
        assert N < 8 or (want[1] > 0).any(), "the case has no ties"
        for P in (1, 3, 64):
            got = rank_scan(q, g, weights, P)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (weights is not None, P)
        if N > 100:
            got = rank_scan(q, g, weights, 3, cuts=[1, 37, N - 5] if N < 1100 else [1, 1025, 2051])
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # the outputs accumulate
    out = torch.zeros(2, Q + GUARD, dtype=torch.int64, device=dev())
    rank_scan(q, g, None, 3, into=out)
    twice = rank_scan(q, g, None, 3, into=out)
    assert np.array_equal(twice[0], 2 * R.rank_counts(q, g)[0]) and np.array_equal(twice[1], 2 * R.rank_counts(q, g)[1])


def test_rank_scan_compares_as_ieee_does():
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, np.float32(1e-45), 3.4e38], dtype=np.float32)
    q = np.concatenate([special, R.quarters(60, 7507)])
    g = np.concatenate([R.quarters(70, 7509), special, special])
    w = np.arange(1, len(g) + 1)
    for weights in (None, w):
        want = R.rank_counts(q, g, weights)
        got = rank_scan(q, g, weights, 3)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[0][0] == 0 and got[1][0] == 0, "a NaN query counts nowhere"
    assert rank_scan(special[3:5], special, None, 1)[1].tolist() == [2, 2], "-0 == 0"


# ================================================================================================ the Python layer
def result_equal(a, b):
    """torch.equal on every tensor, == on every number; a NaN (an empty bin) equals a NaN in the same place"""
    def eq(x, y):
        if not torch.is_tensor(x):
            return x == y or (x != x and y != y)
        if x.is_floating_point():
            return torch.equal(x.isnan(), y.isnan()) and torch.equal(x.nan_to_num(nan=-5.0), y.nan_to_num(nan=-5.0))
        return torch.equal(x, y)
    return all(eq(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("kind,K", [("logit", 10), ("prob", 100)])
def test_reliability_does_not_depend_on_the_batching_and_matches_the_restatement(kind, K):
    N = 130
    code = S.calibration.KINDS[kind]
    x, label = (R.logits if kind == "logit" else R.probabilities)(N, K, 2.0, 7601)
    label[7], x[9, 0] = K + 3, np.nan                      # a foreign label and a row that is not finite
    dx, dl = f32(x), i64(label)
    results = []
    for batch in (1, 37, N):
        rel = S.Reliability(K)
        for i in range(0, N, batch):
            rel.update(dx[i:i + batch], dl[i:i + batch], kind=kind, temperature=1.5)
        assert len(rel) == N
        results.append((rel.result(), rel.result(adaptive=True)))
    assert all(result_equal(r[0], results[0][0]) and result_equal(r[1], results[0][1]) for r in results[1:])
    # against the restatement, fed with the GPU's own per-row values
    rows = calib_rows(x, K, K, code, 1.5, label)
    res = results[0][0]
    state = R.accum(rows["conf"], rows["pred"], label, rows["nll"], rows["brier"], rows["entropy"], K, R.uniform_edges(15),
                    S.calibration.partials(1, N))
    out, diagram = R.finish(*state)
    assert res.n == N - 2 and np.array_equal(res.bin_count.numpy(), state[0])
    assert within_one_ulp(np.array(res[:7], dtype=np.float32), out[:7])
    assert within_one_ulp(res.bin_accuracy.numpy(), diagram[0]) and within_one_ulp(res.bin_confidence.numpy(), diagram[1])
    assert np.array_equal(res.edges.numpy(), R.uniform_edges(15))
    # the adaptive edges hold equal counts +- 1 (the confidences are distinct)
    ada = results[0][1]
    assert len(np.unique(rows["conf"][rows["pred"] >= 0])) == N - 1
    assert ada.bin_count.sum() == N - 2 and int(ada.bin_count.max() - ada.bin_count.min()) <= 1
    assert ada.accuracy == res.accuracy and ada.nll == res.nll


def test_row_stats_update_step_and_detection_replay_from_a_graph():
    """torch.cuda.graph refuses a capture that synchronises with the host.  The four calls are captured whole and replayed on new
    inputs, and on a refitted temperature written to the device"""
    N, K = 257, 10
    cases = [R.logits(N, K, 3.0, s) for s in (7611, 7613)]
    scores = [R.detection_case(s) for s in (7615, 7617)]
    sx, sl = f32(cases[0][0]), i64(cases[0][1])
    ss, sp = f32(scores[0][0]), i64(scores[0][1])
    temp = f32(np.array([1.0]))
    rel = S.Reliability(K).reserve(N, dev())
    ts = S.TemperatureScaler().reset(dev())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                           # warm-up outside the capture
        S.row_stats(sx, sl, temperature=temp)
        rel.update(sx, sl, temperature=temp)
        ts.step(sx, sl)
        S.detection_metrics(ss, sp)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    rel.n = 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stats = S.row_stats(sx, sl, temperature=temp)
        rel.update(sx, sl, temperature=temp)
        step = ts.step(sx, sl)
        det = S.detection_metrics(ss, sp)
    for (x, label), (score, positive), T in ((cases[1], scores[1], 2.5), (cases[0], scores[0], 0.75)):
        sx.copy_(f32(x)), sl.copy_(i64(label)), ss.copy_(f32(score)), sp.copy_(i64(positive))
        temp.fill_(T)
        ts.beta.fill_(0.8)
        graph.replay()
        torch.cuda.synchronize()
        eager = S.row_stats(f32(x), i64(label), temperature=T)
        assert all(torch.equal(a, b) for a, b in zip(stats, eager))
        other = S.Reliability(K)
        other.update(f32(x), i64(label), temperature=T)
        assert result_equal(rel.result(), other.result())
        one = S.TemperatureScaler().reset(dev())
        one.beta.fill_(0.8)
        want_step = one.step(f32(x), i64(label))
        assert torch.equal(step, want_step) and torch.equal(ts.beta, one.beta) and torch.equal(ts.temperature, one.temperature)
        assert all(torch.equal(a, b) for a, b in zip(det, S.detection_metrics(f32(score), i64(positive))))
    assert not torch.equal(S.row_stats(f32(cases[0][0]), temperature=2.5).conf, S.row_stats(f32(cases[0][0]), temperature=0.75).conf)


def test_detection_and_selective_metrics_match_the_restatement():
    score, positive = R.detection_case()
    for tpr in (0.95, 0.5):
        want = R.detection(score, positive, tpr)
        got = S.detection_metrics(f32(score), i64(positive), tpr=tpr)
        for name in want:
            assert abs(float(getattr(got, name)) - want[name]) <= 1e-12, name
    withnan = np.concatenate([score, [np.nan, np.nan]]).astype(np.float32)
    got = S.detection_metrics(f32(withnan), i64(np.concatenate([positive, [1, 0]])))
    assert all(abs(float(getattr(got, name)) - R.detection(score, positive)[name]) <= 1e-12 for name in want)
    one_sided = S.detection_metrics(f32(score), i64(np.ones_like(positive)))
    assert all(bool(torch.isnan(v)) for v in (one_sided.auroc, one_sided.aupr_neg, one_sided.fpr_at_tpr)) and float(one_sided.aupr) == 1.0
    # selective prediction: tied confidences (quarters) and tie-free ones
    rng = np.random.RandomState(7621)
    for conf in (R.quarters(387, 7623, 0.0, 1.0), rng.permutation(300).astype(np.float32) / 300.0):
        correct = (rng.uniform(size=len(conf)) < 0.3 + 0.6 * conf).astype(np.int64)
        want = R.selective(conf, correct)
        got = S.selective_metrics(f32(conf), i64(correct))
        assert abs(float(got.aurc) - want["aurc"]) <= 1e-12 and abs(float(got.e_aurc) - want["e_aurc"]) <= 1e-12
    gt, eq = S.rank_counts(f32(score[:65]), f32(score), i64(positive))
    want = R.rank_counts(score[:65], score, positive)
    assert np.array_equal(gt.cpu().numpy(), want[0]) and np.array_equal(eq.cpu().numpy(), want[1])


# ================================================================================================ evaluate_calibration / evaluate_detection
_MODELS = {}


def eval_model(kind):
    m = _MODELS.get(kind)
    if m is None:
        if kind == "svhn":
            m = S.svhn_VAE((3, 32, 32), {"cont": 32, "disc": [KR.EVAL_CLASSES]}, compute_dtype="fp32")
            m.load_state_dict(KR.eval_state(kind))
        elif kind == "classifier":
            m = S.get_wide_resnet("wideresnet-10-1", 0, input_channels=3, num_classes=KR.EVAL_CLASSES, small_input=True, data_parallel=False,
                                  compute_dtype="fp32")
            m.load_state_dict(Q.make_state("wideresnet-10-1", KR.EVAL_CLASSES))
        else:
            m = S.VariationalAutoEncoder(kind, num_input_channels=3, img_size=(32, 32), data_parallel=False, continuous_latent_dim=128,
                                         disc_latent_dim=KR.EVAL_CLASSES, small_input=True, compute_dtype="fp32")
            m.load_state_dict(KR.eval_state(kind))
        m = _MODELS[kind] = m.cuda().eval()
    return m


def posterior_of(kind, model, image):
    if kind == "svhn":
        return model.classify(image)[0], "prob"
    if kind == "classifier":
        with torch.no_grad():
            return model(image), "logit"
    return model.encode(image)[2], "logit"


@pytest.mark.parametrize("kind", ["wideresnet-10-1", "svhn", "classifier"])
def test_evaluate_calibration_is_the_composition_of_the_public_calls(kind):
    """the models are untrained (closed-form weights): the confidences are near uniform and the numbers mean nothing; the check is the
    equality.  chunk_rows = 16 regroups every batching into the batches the composition uses: the encoders' rows differ in the last bit
    between batch sizes (taking 12-row batches as they come gave ece 0.014294126 against 0.014294125)"""
    model = eval_model(kind)
    _, _, images, labels = (t.to(dev()) for t in KR.eval_images(kind))
    labels = labels.clone()
    labels[5] = -1
    batches = lambda B: [(images[i:i + B], labels[i:i + B]) for i in range(0, images.shape[0], B)]          # noqa: E731
    for adaptive, temperature in ((False, None), (True, 2.0)):
        res = S.evaluate_calibration(model, batches(16), bins=10, adaptive=adaptive, temperature=temperature, chunk_rows=None)
        rel = S.Reliability(KR.EVAL_CLASSES, bins=10)
        for image, label in batches(16):
            x, k = posterior_of(kind, model, image)
            rel.update(x, label, kind=k, temperature=temperature)
        assert result_equal(res, rel.result(adaptive=adaptive))
        for B in (12, 5, 48):
            assert result_equal(res, S.evaluate_calibration(model, batches(B), bins=10, adaptive=adaptive, temperature=temperature,
                                                            chunk_rows=16)), B
        assert res.n == KR.EVAL_TEST - 1 and res.bin_count.sum() == res.n and 0.0 <= res.ece <= 1.0 and res.confidence >= 1.0 / KR.EVAL_CLASSES
    x, k = posterior_of(kind, model, images)
    stats = S.row_stats(x, labels, kind=k)
    valid = labels >= 0
    assert abs(res.accuracy - float((stats.pred[valid] == labels[valid]).double().mean())) <= 1e-7


@pytest.mark.parametrize("kind,score", [("wideresnet-10-1", "msp"), ("wideresnet-10-1", "elbo"), ("svhn", "msp"), ("classifier", "entropy")])
def test_evaluate_detection_is_detection_metrics_over_the_same_scores(kind, score):
    model = eval_model(kind)
    inside = KR.eval_images(kind)[2].to(dev())
    noise = CF.uniform((32, 3, 32, 32), 7701, 0.0, 1.0).to(dev())          # (the closed-form images are smooth fields)
    crit = S.VAECriterion(discrete_dim=KR.EVAL_CLASSES, x_sigma=1.0, bce_reconstruction=True) if score == "elbo" else None
    batches = [inside[:16], inside[16:], noise[:20], noise[20:]]
    got = S.evaluate_detection(model, [batches[0], (batches[1], None)], batches[2:], score=score, criterion=crit)
    values = []
    for image in batches:
        if score == "elbo":
            values.append(model.score_terms(image, crit, ("elbo",))["elbo"])
        else:
            x, k = posterior_of(kind, model, image)
            stats = S.row_stats(x, kind=k)
            values.append(stats.conf if score == "msp" else -stats.entropy)
    flags = torch.cat([torch.ones(len(inside), dtype=torch.int64), torch.zeros(len(noise), dtype=torch.int64)]).to(dev())
    want = S.detection_metrics(torch.cat(values), flags)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert 0.0 <= float(got.auroc) <= 1.0 and 0.0 <= float(got.fpr_at_tpr) <= 1.0
