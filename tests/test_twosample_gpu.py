"""Kernel two-sample statistics on a real MI355X: sv_ksum_scan and sv_ksum_finish through the C ABI -- against the float64 restatement of
tests/_twosample_ref.py by the 8x rule, exact where the arithmetic is (pair counts at a = 0, integer data), `part` bit-equal to the
restatement that walks the kernel's order, batching, cuts, special values --, then the Python layer (shot_vae_amd.twosample).

Allowances are derived, never taken from a GPU result: R.allowance is 8 x the error of the fp32 restatement (the kernel's fp32 pair
values, float64 kernel function and sums) against float64; mmd2 / witness / kid / the permutation statistics propagate it through
their combinations.  Outputs carry guard elements.

Bit-equality and exp: IMQ and POLY use correctly rounded operations only, and numpy restates them bit for bit.  The double exp of two
correct math libraries may differ in the last bit, so the RBF case takes exp's values from the kernel itself -- one launch with S = N
one-hot weight vectors returns k(q_i, g_j) pair by pair; they are held to numpy's exp within 4 ulp -- and checks the ORDER of the sums
bit for bit with them.

Measured on an MI355X (the FIG lines this file prints; DESIGN.md 4o has the table): the kernel's error equals the fp32 restatement's
in every value case, 2.0e-8 .. 5.3e-7 for RBF / IMQ (allowances 1.3e-7 .. 4.2e-6), 2.2e-8 .. 8.7e-5 for POLY (1.8e-7 .. 7.0e-4); the
kernel's exp within 1.00 ulp of numpy's (2.00 over five scales); the gallery cut 1 + 64 + 65: 5.9e-7 (4.7e-6); mmd2 within 3.1e-10 ..
1.2e-8 (2.2e-7 .. 2.2e-6), witness 6.7e-9 .. 5.6e-8 (7.5e-8 .. 4.9e-7), kid values 1.7e-8 (1.7e-6), permutation statistics 6.4e-9
(5.9e-7) with p = 0.30; evaluate_two_sample mmd2 0.200 / 0.0127 within 5.9e-11 / 3.1e-10 (1.5e-7 / 2.2e-7)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import shot_vae_amd as S                                        # noqa: E402
from shot_vae_amd import _lib as L                              # noqa: E402
from shot_vae_amd import aggregate as AG                        # noqa: E402
from shot_vae_amd import twosample as TS                        # noqa: E402
from tests import _knn_ref as KR                                # noqa: E402
from tests import _twosample_ref as R                           # noqa: E402

GUARD = 5
SENTINEL = -7.0


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


def guarded(n, fill=SENTINEL):
    return torch.full((n + 2 * GUARD,), fill, dtype=torch.float64, device=dev())


def unguard(buf, n, what):
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all()), "%s was written beside its end" % what
    return buf[GUARD:GUARD + n]


def raw_scan(kind, kp, degree, dq, Q, q_stride, dg, dw, N, g_stride, w_stride, D, S_=1, col0=0, self0=-1, P=1):
    """one sv_ksum_scan -> part, a float64 device tensor [S, P, Q] (a view into a guarded buffer that is checked)"""
    dk = f64(kp)
    buf = guarded(S_ * P * Q)
    L.call("sv_ksum_scan", kind, p(dk), kp.shape[0], degree, p(dq), Q, q_stride, p(dg), p(dw), N, g_stride, w_stride, D, S_, col0, self0, P,
           p(buf[GUARD:]), st())
    torch.cuda.synchronize()
    return unguard(buf, S_ * P * Q, "part").view(S_, P, Q)


def raw_finish(part, accumulate=0, into=None, q_w=None, w_stride=0, want_total=True):
    """sv_ksum_finish -> (row_sum [S, Q], total [S] or None) float64 numpy"""
    S_, P, Q = part.shape
    part = part.contiguous()
    rows = guarded(S_ * Q)
    if into is not None:
        rows[GUARD:GUARD + S_ * Q] = f64(into).reshape(-1)
    tot = guarded(S_) if want_total else None
    L.call("sv_ksum_finish", p(part), S_, P, Q, accumulate, p(rows[GUARD:]), p(q_w), w_stride, p(tot[GUARD:]) if want_total else None, st())
    torch.cuda.synchronize()
    return (unguard(rows, S_ * Q, "row_sum").view(S_, Q).cpu().numpy(),
            unguard(tot, S_, "total").cpu().numpy() if want_total else None)


def sums(kind, kp, degree, q, g, w=None, col0=0, self0=-1, P=None):
    """scan + finish of one problem from numpy rows -> (row_sum [Q] numpy, part [P, Q] numpy)"""
    Q, D = q.shape
    N = g.shape[0]
    P = P or AG.partials(-(-Q // 64), N)
    part = raw_scan(kind, kp, degree, f32(q), Q, 0, f32(g), None if w is None else f32(w), N, 0, 0, D, 1, col0, self0, P)
    return raw_finish(part, want_total=False)[0][0], part[0].cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def mixed_weights(N, seed):
    """fp32 weights with zeros, negative values and ordinary ones"""
    w = np.random.RandomState(seed).randn(N).astype(np.float32).astype(np.float64)
    w[::5] = 0.0
    return w


# ================================================================================================ values
def test_the_fp32_pair_values_are_sv_pairdists():
    """the restatement's fmaf emulation against the hardware's: sv_pairdist's euclid matrix, bit for bit"""
    for Q, N, D in R.SHAPES:
        q, g = R.case_rows(Q, N, D)
        got = S.pairwise_distance(f32(q), None, f32(g), None, "euclid").cpu().numpy()
        assert np.array_equal(got.view(np.int32), R.pair_values32(R.RBF, q, g).view(np.int32)), (Q, N, D)


@pytest.mark.parametrize("name,n_scale,degree", R.KERNELS)
@pytest.mark.parametrize("Q,N,D", R.SHAPES)
def test_row_sums_against_float64_by_the_8x_rule(Q, N, D, name, n_scale, degree):
    q, g = R.case_rows(Q, N, D)
    kind, kp = R.KIND[name], R.case_params(name, n_scale, degree, q, g)
    for label, w, self0 in (("plain", None, -1), ("weights", mixed_weights(N, 4320), -1), ("self", None, 0)):
        want = R.dense_sums(kind, kp, degree, q, g, w, self0=self0)
        tol, err32 = R.allowance(kind, kp, degree, q, g, w, self0=self0)
        got, _ = sums(kind, kp, degree, q, g, w, self0=self0)
        err = float(np.abs(got - want).max())
        print("FIG ksum %s n_scale=%d degree=%d Q=%d N=%d D=%d %s: err %.3e allowance %.3e (fp32 restatement %.3e) max |sum| %.3e" % (
            name, n_scale, degree, Q, N, D, label, err, tol, err32, float(np.abs(want).max())))
        assert err <= tol


@pytest.mark.parametrize("Q,N,D", R.SHAPES)
def test_rbf_with_a_zero_counts_the_pairs(Q, N, D):
    q, g = R.case_rows(Q, N, D)
    kp = R.params(R.RBF, [0.0])
    for P in (1, 3):
        assert np.array_equal(sums(R.RBF, kp, 0, q, g, P=P)[0], np.full(Q, float(N)))
    x = g
    assert np.array_equal(sums(R.RBF, kp, 0, x, x, self0=0)[0], np.full(N, float(N - 1)))
    assert np.array_equal(sums(R.RBF, R.params(R.RBF, [0.0] * 5), 0, x, x, self0=0, P=2)[0], np.full(N, float(N - 1)))
    assert np.array_equal(sums(R.IMQ, R.params(R.IMQ, [0.0]), 0, x, x, self0=0, P=2)[0], np.full(N, float(N - 1)))
    if N > 2:                                                   # the queries are rows 2 .. of the gallery
        assert np.array_equal(sums(R.RBF, kp, 0, x[2:], x, self0=2)[0], np.full(N - 2, float(N - 1)))


@pytest.mark.parametrize("D", (7, 130))
def test_integer_data_under_the_cubic_kernel_is_exact(D):
    rs = np.random.RandomState(4330 + D)
    q, g = rs.randint(-8, 9, (70, D)).astype(np.float64), rs.randint(-8, 9, (130, D)).astype(np.float64)
    kp = R.params(R.POLY, 1.0, 1.0)
    K = (q.astype(np.int64) @ g.astype(np.int64).T + 1) ** 3    # |u| <= 64 D: the cube and the sums are far below 2^53
    for P in (1, 2, 3):
        assert np.array_equal(sums(R.POLY, kp, 3, q, g, P=P)[0], K.sum(axis=1).astype(np.float64))
    w = rs.randint(-3, 4, 130).astype(np.float64)
    assert np.array_equal(sums(R.POLY, kp, 3, q, g, w)[0], (K * w.astype(np.int64)[None, :]).sum(axis=1).astype(np.float64))
    x = g
    Kx = (x.astype(np.int64) @ x.astype(np.int64).T + 1) ** 3
    assert np.array_equal(sums(R.POLY, kp, 3, x, x, self0=0)[0], (Kx.sum(axis=1) - np.diag(Kx)).astype(np.float64))


# ================================================================================================ the order of the sums
def device_kernel_values(kind, kp, degree, q, g):
    """k(q_i, g_j) [Q, N] as the kernel evaluates it: ONE launch with S = N one-hot weight vectors over shared rows (a weight of 0
    adds an exact 0 to a finite sum)"""
    Q, D = q.shape
    N = g.shape[0]
    eye = torch.eye(N, dtype=torch.float32, device=dev()).contiguous()
    part = raw_scan(kind, kp, degree, f32(q), Q, 0, f32(g), eye, N, 0, N, D, N, 0, -1, 1)
    return part[:, 0, :].t().contiguous().cpu().numpy()


@pytest.mark.parametrize("P", (1, 2, 7, 64))
def test_part_is_bit_equal_to_the_kernel_order_restatement(P):
    """P = 64 at N = 65: 62 of the 64 states own no tile and hold 0"""
    Q, N, D = 33, 65, 128
    q, g = R.case_rows(Q, N, D)
    w = mixed_weights(N, 4340)
    for name, n_scale, degree in R.KERNELS:
        kind, kp = R.KIND[name], R.case_params(name, n_scale, degree, q, g)
        K = None
        if name == "rbf":
            K = device_kernel_values(kind, kp, degree, q, g)
            ref = R.kernel_matrix(kind, kp, degree, q, g, fp32=True)
            ulp = float((np.abs(K - ref) / np.spacing(ref)).max())
            print("FIG ksum rbf n_scale=%d: the kernel's exp against numpy's, %.2f ulp at most" % (n_scale, ulp))
            assert ulp <= 4.0 * n_scale
        for wv, self0 in ((None, -1), (w, 3)):
            want = R.ordered_parts(kind, kp, degree, q, g, wv, self0=self0, P=P, K=K)
            got = sums(kind, kp, degree, q, g, wv, self0=self0, P=P)[1]
            assert same_bits(got, want), (name, n_scale, degree, P, self0)
            if P == 64:
                assert not got[2:].any()


def test_a_second_shape_in_kernel_order():
    """two query tiles, three gallery tiles, D no multiple of 16, the gallery offset by col0"""
    q, g = R.case_rows(70, 130, 17)
    w = mixed_weights(130, 4342)
    for name, n_scale, degree in (("imq", 5, 0), ("poly", 1, 3)):
        kind, kp = R.KIND[name], R.case_params(name, n_scale, degree, q, g)
        for P in (1, 2):
            want = R.ordered_parts(kind, kp, degree, q, g, w, col0=40, self0=45, P=P)
            got = sums(kind, kp, degree, q, g, w, col0=40, self0=45, P=P)[1]
            assert same_bits(got, want), (name, P)


# ================================================================================================ batching and cuts
def test_three_problems_with_every_stride_shared_or_dense():
    Q, N, D, S_ = 70, 130, 17, 3
    qs = [R.rows(Q, D, 4350 + s) for s in range(S_)]
    gs = [R.rows(N, D, 4360 + s) for s in range(S_)]
    ws = [mixed_weights(N, 4370 + s) for s in range(S_)]
    kind, kp = R.IMQ, R.params(R.IMQ, [0.02, 0.05])
    P = 2
    one = lambda q, g, w: sums(kind, kp, 0, q, g, w, self0=1, P=P)[1]          # noqa: E731
    for dense_q, dense_g, dense_w in ((1, 0, 0), (0, 1, 1), (1, 1, 1), (0, 0, 1), (0, 0, 0), (1, 1, None)):
        dq = f32(np.stack(qs)) if dense_q else f32(qs[0])
        dg = f32(np.stack(gs)) if dense_g else f32(gs[0])
        dw = None if dense_w is None else (f32(np.stack(ws)) if dense_w else f32(ws[0]))
        part = raw_scan(kind, kp, 0, dq, Q, Q * D if dense_q else 0, dg, dw, N, N * D if dense_g else 0, N if dense_w else 0, D, S_, 0, 1, P)
        for s in range(S_):
            want = one(qs[s if dense_q else 0], gs[s if dense_g else 0], None if dense_w is None else ws[s if dense_w else 0])
            assert same_bits(part[s].cpu().numpy(), want), (dense_q, dense_g, dense_w, s)
    # strides larger than the arrays: the problems sit in a padded buffer
    big = torch.full((S_, Q * D + 11), float("nan"), dtype=torch.float32, device=dev())
    for s in range(S_):
        big[s, :Q * D] = f32(qs[s]).reshape(-1)
    part = raw_scan(kind, kp, 0, big, Q, Q * D + 11, f32(gs[0]), None, N, 0, 0, D, S_, 0, -1, P)
    for s in range(S_):
        assert same_bits(part[s].cpu().numpy(), sums(kind, kp, 0, qs[s], gs[0], P=P)[1])


def test_cuts_and_repeats():
    Q, N, D = 70, 130, 17
    q, g = R.case_rows(Q, N, D)
    w = mixed_weights(N, 4380)
    name, n_scale, degree = "rbf", 5, 0
    kind, kp = R.KIND[name], R.case_params(name, n_scale, degree, q, g)
    whole, part = sums(kind, kp, degree, q, g, w, self0=2, P=2)
    again, part2 = sums(kind, kp, degree, q, g, w, self0=2, P=2)
    assert same_bits(whole, again) and same_bits(part, part2)
    # the gallery cut 1 + 64 + 65 through col0, accumulated in call order: another order of the additions, within the allowance
    tol, _ = R.allowance(kind, kp, degree, q, g, w, self0=2)
    acc = None
    for a, b in ((0, 1), (1, 65), (65, 130)):
        pt = raw_scan(kind, kp, degree, f32(q), Q, 0, f32(g[a:b]), f32(w[a:b]), b - a, 0, 0, D, 1, a, 2, 2)
        acc = raw_finish(pt, accumulate=0 if acc is None else 1, into=acc, want_total=False)[0]
    want = R.dense_sums(kind, kp, degree, q, g, w, self0=2)
    print("FIG ksum gallery cut 1 + 64 + 65: err %.3e against the whole scan %.3e, allowance %.3e" % (
        float(np.abs(acc[0] - want).max()), float(np.abs(whole - want).max()), tol))
    assert np.abs(acc[0] - want).max() <= tol and np.abs(acc[0] - whole).max() <= tol
    # the queries cut 1 + 64 + 5: the same bits
    for a, b in ((0, 1), (1, 65), (65, 70)):
        got = sums(kind, kp, degree, q[a:b], g, w, self0=2 + a, P=2)[0]
        assert same_bits(got, whole[a:b]), (a, b)


# ================================================================================================ special values
def test_special_values_reach_exactly_their_sums():
    Q, N, D = 33, 70, 17
    q, g = R.case_rows(Q, N, D)
    kind, kp = R.IMQ, R.params(R.IMQ, [0.03])
    clean = sums(kind, kp, 0, q, g, P=2)[0]
    # rows beyond Q and N hold NaN in memory: by predicate they reach nothing
    qpad, gpad = np.concatenate([q, np.full((40, D), np.nan)]), np.concatenate([g, np.full((70, D), np.nan)])
    part = raw_scan(kind, kp, 0, f32(qpad), Q, 0, f32(gpad), None, N, 0, 0, D, 1, 0, -1, 2)
    assert same_bits(raw_finish(part, want_total=False)[0][0], clean)
    for bad in (np.nan, np.inf):
        qb, gb = q.copy(), g.copy()
        qb[7] = bad
        got = sums(kind, kp, 0, qb, g, P=2)[0]
        want = R.finish_rows(R.ordered_parts(kind, kp, 0, qb, g, P=2))
        assert np.array_equal(bits(np.delete(got, 7)), bits(np.delete(clean, 7))) and np.array_equal(got, want, equal_nan=True), bad
        assert np.isnan(got[7]) if np.isnan(bad) else got[7] == 0.0          # 1 / (1 + a inf) = 0
        gb[66] = bad
        got = sums(kind, kp, 0, q, gb, P=2)[0]
        want = R.finish_rows(R.ordered_parts(kind, kp, 0, q, gb, P=2))
        assert np.array_equal(got, want, equal_nan=True) and (np.isnan(got).all() if np.isnan(bad) else np.isfinite(got).all()), bad
    # a gallery row that holds a NaN, under a = 0 (every finite pair counts 1): a weight of 0 is a product, so 0 * NaN reaches the row;
    # the self pair is a predicate, so the query that IS that row never reads it
    x = g.copy()
    x[5, 3] = np.nan
    zero = R.params(R.RBF, [0.0])
    w = np.ones(N)
    w[5] = 0.0
    others = np.delete(x, 5, axis=0)
    assert np.isnan(sums(R.RBF, zero, 0, others, x, w)[0]).all()
    got = sums(R.RBF, zero, 0, others[:4], x[5:6], col0=5, self0=5)[0]      # query 0 stands for global row 5: its one pair is left out
    assert got[0] == 0.0 and np.isnan(got[1:]).all()
    # weights: 0, negative, NaN
    w = mixed_weights(N, 4390)
    got = sums(kind, kp, 0, q, g, w, P=2)[0]
    assert same_bits(got, R.finish_rows(R.ordered_parts(kind, kp, 0, q, g, w, P=2)))
    assert (w < 0).any() and (w > 0).any() and (w == 0).any() and not same_bits(got, clean)
    w[64] = np.nan                                              # the second tile: state 1 of 2
    part = sums(kind, kp, 0, q, g, w, P=2)[1]
    assert np.isnan(part[1]).all() and same_bits(part[0], R.ordered_parts(kind, kp, 0, q, g, w, P=2)[0])


# ================================================================================================ sv_ksum_finish
def test_finish_follows_the_restatements_order():
    rs = np.random.RandomState(4400)
    S_, P, Q = 2, 7, 600
    part = rs.randn(S_, P, Q) * 10.0 ** rs.randint(-3, 4, (S_, P, Q))
    qw = rs.randn(S_, Q).astype(np.float32).astype(np.float64)
    dpart = f64(part)
    rows, tot = raw_finish(dpart)
    for s in range(S_):
        assert same_bits(rows[s], R.finish_rows(part[s])) and tot[s] == R.finish_total(rows[s])
    rows_w, tot_w = raw_finish(dpart, q_w=f32(qw), w_stride=Q)
    rows_s, tot_s = raw_finish(dpart, q_w=f32(qw[0]), w_stride=0)
    for s in range(S_):
        assert tot_w[s] == R.finish_total(rows[s], qw[s]) and tot_s[s] == R.finish_total(rows[s], qw[0])
    assert same_bits(rows_w, rows) and same_bits(rows_s, rows)
    assert same_bits(raw_finish(dpart, want_total=False)[0], rows)            # a NULL total: the rows are the same bits
    base = rs.randn(S_, Q)
    acc = raw_finish(dpart, accumulate=1, into=base)[0]
    for s in range(S_):
        assert same_bits(acc[s], R.finish_rows(part[s], into=base[s]))
    part[1, 3, 17] = np.nan
    rows, tot = raw_finish(f64(part))
    assert np.isnan(rows[1, 17]) and np.isnan(tot[1]) and not np.isnan(rows[0]).any() and not np.isnan(tot[0])
    assert int(np.isnan(rows).sum()) == 1
    one = raw_finish(f64(rs.randn(1, 1, 1)))                    # Q = 1: 255 threads add nothing
    assert one[1][0] == one[0][0, 0]


# ================================================================================================ the Python layer
def test_kernel_sums_equals_the_calls_by_hand_and_a_replayed_graph():
    Q, N, D = 70, 130, 17
    q, g = R.case_rows(Q, N, D)
    w = mixed_weights(N, 4410)
    a = float(R.median_bandwidth(np.concatenate([q, g])))
    for kernel, gamma, degree, kp in (("rbf", a, 3, R.params(R.RBF, [a])), ("imq", [a, 2 * a], 3, R.params(R.IMQ, [a, 2 * a])),
                                      ("poly", None, 2, R.params(R.POLY, 1.0 / D, 1.0))):
        got, tot = TS.kernel_sums(f32(q), f32(g), kernel, gamma, degree=degree, weights=f32(w), exclude_self_from=4, total=True)
        assert got.dtype == torch.float64 and tuple(got.shape) == (Q,) and tot.dtype == torch.float64 and tot.dim() == 0
        P = AG.partials(-(-Q // 64), N)
        part = raw_scan(R.KIND[kernel], kp, degree, f32(q), Q, 0, f32(g), f32(w), N, 0, 0, D, 1, 0, 4, P)
        rows, total = raw_finish(part)
        assert same_bits(got.cpu().numpy(), rows[0]) and float(tot) == total[0], kernel
    ladder = TS.kernel_sums(f32(q), f32(g), "rbf", a, scales=R.LADDER)
    assert same_bits(ladder.cpu().numpy(), sums(R.RBF, R.params(R.RBF, a * np.asarray(R.LADDER)), 0, q, g)[0])
    # under graph capture, replayed on new inputs; the bandwidth is a device tensor
    da = torch.tensor([a], dtype=torch.float64, device=dev())
    qs = [f32(q), f32(R.rows(Q, D, 4412))]
    sq = qs[0].clone()
    dg = f32(g)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                               # warm-up outside the capture
        TS.kernel_sums(sq, dg, "rbf", da)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = TS.kernel_sums(sq, dg, "rbf", da)
    for x in (qs[1], qs[0]):
        sq.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(got, TS.kernel_sums(x, dg, "rbf", da)) and float(got.sum()) > 0.0
    assert not torch.equal(TS.kernel_sums(qs[0], dg, "rbf", da), TS.kernel_sums(qs[1], dg, "rbf", da))


def test_median_bandwidth_names_the_restatements_element(monkeypatch):
    x, y = R.rows(40, 17, 4420), R.rows(31, 17, 4422)
    reads = []
    for name in ("cpu", "item", "tolist"):
        monkeypatch.setattr(torch.Tensor, name, (lambda real: lambda self, *a, **k: (reads.append(1), real(self, *a, **k))[1])(getattr(torch.Tensor, name)))
    a = TS.median_bandwidth(f32(x), f32(y))
    sub = TS.median_bandwidth(f32(x), f32(y), max_rows=30, seed=5)
    lad = TS.median_bandwidth(f32(x), scales=(0.5, 1.0, 2.0))
    monkeypatch.undo()
    assert not reads, "median_bandwidth read from the device"
    assert a.dtype == torch.float64 and a.dim() == 0 and a.is_cuda

    def element(rows):                                          # from the device's own fp32 matrix, read back
        d = S.pairwise_distance(f32(rows), None, f32(rows), None, "euclid").double().cpu().numpy()
        return 1.0 / R.lower_median(d[~np.eye(len(d), dtype=bool)])
    pooled = np.concatenate([x, y])
    assert float(a) == element(pooled)
    assert abs(float(a) - R.median_bandwidth(pooled)) <= 1e-5 * float(a)
    pick = torch.randperm(71, generator=torch.Generator().manual_seed(5))[:30].numpy()
    assert float(sub) == element(pooled[pick]) and float(sub) != float(a)
    assert lad.tolist() == [0.5 * element(x), element(x), 2.0 * element(x)]


@pytest.mark.parametrize("kernel,n_scale,degree", [("rbf", 1, 3), ("rbf", 5, 3), ("imq", 1, 3), ("poly", 1, 3)])
def test_mmd2_and_witness_against_float64(kernel, n_scale, degree):
    D = 17
    x, y = R.rows(70, D, 4430), (R.rows(63, D, 4432) * 1.2 + 0.2).astype(np.float32).astype(np.float64)
    at = R.rows(33, D, 4434)
    kind = R.KIND[kernel]
    kp = R.case_params(kernel, n_scale, degree, x, y)
    gamma = None if kernel == "poly" else f64(kp)               # the parameter array itself
    for unbiased in (True, False):
        got = TS.mmd2(f32(x), f32(y), kernel, gamma, degree=degree, unbiased=unbiased)
        assert got.dtype == torch.float64 and got.dim() == 0 and got.is_cuda
        want, tol = R.mmd2(kind, kp, degree, x, y, unbiased), R.mmd2_allowance(kind, kp, degree, x, y, unbiased)
        print("FIG mmd2 %s n_scale=%d unbiased=%s: got %.9e want %.9e err %.2e allowance %.2e" % (
            kernel, n_scale, unbiased, float(got), want, abs(float(got) - want), tol))
        assert abs(float(got) - want) <= tol and float(got) > 100.0 * tol
    same = TS.mmd2(f32(x), f32(x), kernel, gamma, degree=degree, unbiased=False)
    assert abs(float(same)) <= R.mmd2_allowance(kind, kp, degree, x, x, False)
    got = TS.witness(f32(x), f32(y), f32(at), kernel, gamma, degree=degree).cpu().numpy()
    want = R.witness(kind, kp, degree, x, y, at)
    tol = R.allowance(kind, kp, degree, at, x)[0] / len(x) + R.allowance(kind, kp, degree, at, y)[0] / len(y)
    print("FIG witness %s n_scale=%d: err %.2e allowance %.2e" % (kernel, n_scale, float(np.abs(got - want).max()), tol))
    assert np.abs(got - want).max() <= tol
    if kernel == "rbf" and n_scale == 1:                        # "median": the device's own bandwidth of the pooled rows
        a = float(TS.median_bandwidth(f32(x), f32(y)))
        assert float(TS.mmd2(f32(x), f32(y))) == float(TS.mmd2(f32(x), f32(y), "rbf", a))


def test_kid_against_the_restatement_on_the_same_index_sets(monkeypatch):
    real, fake = R.rows(130, 17, 4440), (R.rows(130, 17, 4442) * 1.1 + 0.1).astype(np.float32).astype(np.float64)
    reads = []
    for name in ("cpu", "item", "tolist"):
        monkeypatch.setattr(torch.Tensor, name, (lambda real_: lambda self, *a, **k: (reads.append(1), real_(self, *a, **k))[1])(getattr(torch.Tensor, name)))
    res = TS.kid(f32(real), f32(fake), subsets=4, subset_size=50, seed=3, return_indices=True)
    monkeypatch.undo()
    assert len(reads) == 1, "kid() reads the host once"
    assert res["subsets"] == 4 and res["subset_size"] == 50 and res["clipped"] is False
    ia, ib = (t.cpu().numpy() for t in res["indices"])
    assert ia.shape == ib.shape == (4, 50) and all(len(set(r)) == 50 for r in ia) and all(len(set(r)) == 50 for r in ib)
    want_ia, want_ib = TS.subset_indices(130, 130, 4, 50, 3)
    assert np.array_equal(ia, want_ia.numpy()) and np.array_equal(ib, want_ib.numpy())
    mean, std, vals = R.kid(real, fake, ia, ib)
    tol = R.kid_allowance(real, fake, ia, ib)
    err = float(np.abs(res["values"].cpu().numpy() - vals).max())
    print("FIG kid 4 x 50 of 130 x 17: mean %.9e (restatement %.9e) std %.9e (%.9e) value err %.2e allowance %.2e" % (
        res["kid_mean"], mean, res["kid_std"], std, err, tol))
    assert err <= tol and abs(res["kid_mean"] - mean) <= tol and abs(res["kid_std"] - std) <= 2.0 * tol
    assert res["kid_mean"] > 100.0 * tol
    small = TS.kid(f32(real[:30]), f32(fake), subsets=2, subset_size=50, seed=3)
    assert small["subset_size"] == 30 and small["clipped"] is True


def count_bracket(stats, tol):
    """(sure, undecided): permuted statistics above the observed one by more than twice the allowance, and within it"""
    d = stats[1:] - stats[0]
    return int(np.sum(d > 2.0 * tol)), int(np.sum(np.abs(d) <= 2.0 * tol))


def test_permutation_test_with_given_signs(monkeypatch):
    x, y, signs = R.permutation_case()
    B = R.PERM_B
    a = float(TS.median_bandwidth(f32(x), f32(y)))
    kp = R.params(R.RBF, [a])
    reads = []
    for name in ("cpu", "item", "tolist"):
        monkeypatch.setattr(torch.Tensor, name, (lambda real: lambda self, *a_, **k: (reads.append(1), real(self, *a_, **k))[1])(getattr(torch.Tensor, name)))
    res = TS.permutation_test(f32(x), f32(y), "rbf", a, signs=torch.from_numpy(signs).to(dev()))
    monkeypatch.undo()
    assert len(reads) == 1, "permutation_test() reads the host once"
    want = R.permutation_stats(R.RBF, kp, 0, x, y, signs)
    tol = R.permutation_allowance(R.RBF, kp, 0, x, y)
    err = float(np.abs(res["statistics"] - want).max())
    print("FIG permutation_test %d + %d rows x %d splits: statistic %.9e err %.2e allowance %.2e p %.4f" % (
        R.PERM_N, R.PERM_M, B, res["statistic"], err, tol, res["p_value"]))
    assert res["statistics"].shape == (B + 1,) and err <= tol
    sure, undecided = count_bracket(want, tol)
    count = round(res["p_value"] * (B + 1)) - 1
    assert sure <= count <= sure + undecided and undecided <= 0.02 * B
    assert abs(res["statistic"] - float(TS.mmd2(f32(x), f32(y), "rbf", a, unbiased=False))) <= 2.0 * tol
    # drawn splits: the same seed gives the same result, every split keeps n rows in the first group
    r1 = TS.permutation_test(f32(x), f32(y), "rbf", a, permutations=20, seed=9)
    r2 = TS.permutation_test(f32(x), f32(y), "rbf", a, permutations=20, seed=9)
    assert np.array_equal(r1["statistics"], r2["statistics"]) and r1["statistics"][0] == res["statistics"][0]
    # separated blobs: no permuted split reaches the observed statistic
    far = TS.permutation_test(f32(x), f32(y + 3.0), permutations=50, seed=1)
    assert far["p_value"] == 1.0 / 51.0


# ================================================================================================ the evaluators
_MODELS = {}
EVAL_N, EVAL_KEY, EVAL_TAU = 96, 77, 0.9


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


def counting(monkeypatch):
    reads = []
    for name in ("cpu", "item", "tolist"):
        monkeypatch.setattr(torch.Tensor, name, (lambda real: lambda self, *a, **k: (reads.append(1), real(self, *a, **k))[1])(getattr(torch.Tensor, name)))
    return reads


@pytest.mark.parametrize("kind", KR.EVAL_KINDS)
def test_the_evaluators_on_the_closed_form_models(kind, monkeypatch):
    model = eval_model(kind)
    xa, ya, xb, yb = (t.to(dev()) for t in KR.eval_images(kind))
    assert xa.shape[0] == EVAL_N
    xb = (0.8 * xb + 0.1).contiguous()                          # a shifted second set: 48 images
    batches = lambda x, y, b: [(x[i:i + b], y[i:i + b]) for i in range(0, x.shape[0], b)]          # noqa: E731
    host = lambda t: t.double().cpu().numpy()                  # noqa: E731

    # ---- evaluate_two_sample
    reads = counting(monkeypatch)
    res = S.evaluate_two_sample(model, batches(xa, ya, 16), batches(xb, yb, 16), permutations=19, seed=5)
    n_reads = len(reads)
    monkeypatch.undo()
    assert n_reads == 1, "evaluate_two_sample reads the host once (%d)" % n_reads
    again = S.evaluate_two_sample(model, batches(xa, ya, 48), batches(xb, yb, 48), permutations=19, seed=5)
    assert again == res and res["n_a"] == EVAL_N and res["n_b"] == 48
    ma, mb = host(S.encode_posterior(model, xa)[0]), host(S.encode_posterior(model, xb)[0])
    a = float(TS.median_bandwidth(f32(ma), f32(mb)))
    kp = R.params(R.RBF, [a])
    want, tol = R.mmd2(R.RBF, kp, 0, ma, mb, True), R.mmd2_allowance(R.RBF, kp, 0, ma, mb, True)
    gen = torch.Generator().manual_seed(5)
    signs = np.zeros((19, EVAL_N + 48), dtype=bool)
    for b in range(19):
        signs[b, torch.randperm(EVAL_N + 48, generator=gen)[:EVAL_N].numpy()] = True
    stats = R.permutation_stats(R.RBF, kp, 0, ma, mb, signs)
    ptol = R.permutation_allowance(R.RBF, kp, 0, ma, mb)
    sure, undecided = count_bracket(stats, ptol)
    print("FIG evaluate_two_sample %s: mmd2 %.9e (restatement %.9e, err %.2e, allowance %.2e) statistic %.9e (%.9e, allowance %.2e) p %.3f" % (
        kind, res["mmd2"], want, abs(res["mmd2"] - want), tol, res["statistic"], stats[0], ptol, res["p_value"]))
    assert abs(res["mmd2"] - want) <= tol and abs(res["statistic"] - stats[0]) <= ptol
    assert sure <= round(res["p_value"] * 20) - 1 <= sure + undecided
    plain = S.evaluate_two_sample(model, batches(xa, ya, 16), batches(xb, yb, 16))
    assert set(plain) == {"mmd2", "n_a", "n_b"} and plain["mmd2"] == res["mmd2"]

    # ---- evaluate_prior_match
    reads = counting(monkeypatch)
    res = S.evaluate_prior_match(model, batches(xa, ya, 16), samples=2, key=EVAL_KEY)
    n_reads = len(reads)
    monkeypatch.undo()
    assert n_reads == 1, "evaluate_prior_match reads the host once (%d)" % n_reads
    assert S.evaluate_prior_match(model, batches(xa, ya, 48), samples=2, key=EVAL_KEY) == res and res["n"] == 2 * EVAL_N and res["analytic"]
    mu, ls = S.encode_posterior(model, xa)
    agg = S.AggregatePosterior(mu.shape[1])
    z = torch.cat([agg.sample(mu, ls, key=EVAL_KEY, row0=0, s=s)[0] for s in range(2)])
    a = float(TS.median_bandwidth(z))
    kp, zn = R.params(R.RBF, [a]), host(z)
    n = len(zn)
    exy, eyy = R.rbf_prior_expectations(zn, kp)
    want = R.dense_sums(R.RBF, kp, 0, zn, zn, self0=0).sum() / (n * (n - 1)) - 2.0 * exy.mean() + eyy
    tol = R.allowance(R.RBF, kp, 0, zn, zn, self0=0)[0] * n / (n * (n - 1)) + 1e-13
    print("FIG evaluate_prior_match %s: mmd2 %.9e (restatement %.9e, err %.2e, allowance %.2e)" % (kind, res["mmd2"], want, abs(res["mmd2"] - want), tol))
    assert abs(res["mmd2"] - want) <= tol
    imq = S.evaluate_prior_match(model, batches(xa, ya, 16), key=EVAL_KEY, kernel="imq", seed=3)
    assert imq == S.evaluate_prior_match(model, batches(xa, ya, 48), key=EVAL_KEY, kernel="imq", seed=3) and not imq["analytic"]
    prior = torch.randn(EVAL_N, mu.shape[1], generator=torch.Generator(device=dev()).manual_seed(3), device=dev(), dtype=torch.float32)
    z1 = agg.sample(mu, ls, key=EVAL_KEY, row0=0, s=0)[0]
    a = float(TS.median_bandwidth(z1))
    kp = R.params(R.IMQ, [a])
    want, tol = R.mmd2(R.IMQ, kp, 0, host(z1), host(prior), True), R.mmd2_allowance(R.IMQ, kp, 0, host(z1), host(prior), True)
    assert abs(imq["mmd2"] - want) <= tol

    # ---- evaluate_kid
    for source in ("generate", "reconstruct"):
        kw = dict(source=source, subsets=4, subset_size=50, seed=2, key=EVAL_KEY, tau=EVAL_TAU)
        reads = counting(monkeypatch)
        res = S.evaluate_kid(model, batches(xa, ya, 16), **kw)
        n_reads = len(reads)
        monkeypatch.undo()
        assert n_reads == 1, "evaluate_kid reads the host once (%d)" % n_reads
        assert S.evaluate_kid(model, batches(xa, ya, 48), **kw) == res and res["n"] == EVAL_N and res["subset_size"] == 50
        made = model.reconstruct(xa) if source == "reconstruct" else model.generate(ya, EVAL_KEY, tau=EVAL_TAU, row0=0)
        real, fake = host(S.encode_posterior(model, xa)[0]), host(S.encode_posterior(model, made)[0])
        ia, ib = (t.numpy() for t in TS.subset_indices(EVAL_N, EVAL_N, 4, 50, 2))
        mean, std, _ = R.kid(real, fake, ia, ib)
        tol = R.kid_allowance(real, fake, ia, ib)
        print("FIG evaluate_kid %s %s: mean %.9e (restatement %.9e) std %.9e (%.9e) allowance %.2e" % (
            kind, source, res["kid_mean"], mean, res["kid_std"], std, tol))
        assert abs(res["kid_mean"] - mean) <= tol and abs(res["kid_std"] - std) <= 2.0 * tol
