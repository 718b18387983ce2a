"""Label spreading / propagation on a real MI355X: sv_lp_normalize, sv_lp_step and sv_lp_finish through the C ABI against the
restatement of tests/_labelprop_ref.py (pinned to scikit-learn and the closed form by tests/test_labelprop_cpu.py), then the Python
layer (shot_vae_amd.propagate).

sv_lp_step is compared BIT FOR BIT with the restatement that walks the CSR graph in the kernel's order: the products are exact in
double and the additions run in a fixed order, so there is nothing to tolerate.  Where a float64 result of another order is the
reference, the allowance follows the project's 8x rule and is formed when the test runs, never from a GPU result: R.allowance = 8 x
the error of the fp32 numpy restatement against float64 on the case's own inputs (never less than 8 half ulps of fp32 at the largest
value).  Outputs carry guard rows.  The measured figures are in DESIGN.md 4m."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import shot_vae_amd as S                                        # noqa: E402
from shot_vae_amd import _lib as L                              # noqa: E402
from shot_vae_amd import propagate as PG                        # noqa: E402
from tests import _knn_ref as KR                                # noqa: E402
from tests import _labelprop_ref as R                           # noqa: E402
from tests.test_labelprop_cpu import CASES, case                # noqa: E402

GUARD = 3
EPS32 = R.EPS32


def dev():
    return torch.device("cuda:0")


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev())


def i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev())


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def ulps32(a, b):
    """the largest distance of a from the float64 values b in units of fp32 spacing at b"""
    b = np.asarray(b, dtype=np.float64)
    unit = np.spacing(np.maximum(np.abs(b), np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)
    return float((np.abs(np.asarray(a, dtype=np.float64) - b) / unit).max()) if b.size else 0.0


def ulps64(a, b):
    b = np.asarray(b, dtype=np.float64)
    return float((np.abs(np.asarray(a, dtype=np.float64) - b) / np.spacing(np.maximum(np.abs(b), np.finfo(np.float64).tiny))).max()) if b.size else 0.0


# ------------------------------------------------------------------------------------------------ the entry points by hand
def normalize(rowptr, col, val, n, mode):
    """sv_lp_normalize -> (sval fp32 [nnz], deg float64 [n]) numpy; sval starts as -7 (an entry outside every segment keeps it)"""
    nnz = len(col)
    dr, dc, dv = i64(rowptr), i64(col), f32(val)
    sval = torch.full((nnz + GUARD,), -7.0, dtype=torch.float32, device=dev())
    deg = torch.full((n + GUARD,), -7.0, dtype=torch.float64, device=dev())
    L.call("sv_lp_normalize", p(dr), p(dc), p(dv), n, nnz, mode, p(deg), p(sval) if nnz else None, st())
    torch.cuda.synchronize()
    assert bool((sval[nnz:] == -7.0).all()) and bool((deg[n:] == -7.0).all()), "sv_lp_normalize wrote behind its outputs"
    return sval[:nnz].cpu().numpy(), deg[:n].cpu().numpy()


def step(rowptr, col, sval, f_in, n, k, label, variant, alpha=0.2, oma=None, cuts=None, stats=False):
    """sv_lp_step over the rows cut at `cuts` (offset pointers) -> f_out fp32 [n, k] numpy (, stats float64 [2]); guard rows checked"""
    nnz, m = len(col), f_in.shape[0]
    dr, dc, dv, df = i64(rowptr), i64(col), f32(sval), f32(f_in)
    dl = i64(label) if label is not None else None
    out = torch.full((n + GUARD, k), -7.0, dtype=torch.float32, device=dev())
    scratch = torch.full((PG.step_scratch(n, k) + GUARD,), -7.0, dtype=torch.float64, device=dev()) if stats else None
    dstats = torch.full((2 + GUARD,), -7.0, dtype=torch.float64, device=dev()) if stats else None
    edges = [0] + list(cuts or []) + [n]
    for lo, hi in zip(edges[:-1], edges[1:]):
        L.call("sv_lp_step", p(df), m, p(dr[lo:]), p(dc), p(dv), nnz, hi - lo, k, p(dl[lo:]) if dl is not None else None, variant,
               float(alpha), float(1.0 - alpha if oma is None else oma), p(out[lo:]), p(scratch), p(dstats), st())
    torch.cuda.synchronize()
    assert bool((out[n:] == -7.0).all()), "sv_lp_step wrote behind f_out"
    if stats:
        assert bool((scratch[PG.step_scratch(n, k):] == -7.0).all()) and bool((dstats[2:] == -7.0).all()), "sv_lp_step wrote behind its statistics"
        return out[:n].cpu().numpy(), dstats[:2].cpu().numpy()
    return out[:n].cpu().numpy()


def finish(f, want=("proba", "pred", "conf", "counts")):
    """sv_lp_finish -> dict of numpy arrays; an output that was not asked for stays as it was"""
    n, k = f.shape
    df = f32(f)
    t = dict(proba=torch.full((n + GUARD, k), -7.0, dtype=torch.float32, device=dev()), pred=torch.full((n + GUARD,), -7, dtype=torch.int64, device=dev()),
             conf=torch.full((n + GUARD,), -7.0, dtype=torch.float32, device=dev()), counts=torch.full((2 + GUARD,), -7, dtype=torch.int64, device=dev()))
    L.call("sv_lp_finish", p(df), n, k, *[p(t[name]) if name in want else None for name in ("proba", "pred", "conf", "counts")], st())
    torch.cuda.synchronize()
    for name, rows in (("proba", n), ("pred", n), ("conf", n), ("counts", 2)):
        assert bool((t[name][rows:] == -7).all()), "sv_lp_finish wrote behind " + name
        if name not in want:
            assert bool((t[name] == -7).all()), name
    return {name: t[name][:rows].cpu().numpy() for name, rows in (("proba", n), ("pred", n), ("conf", n), ("counts", 2))}


def special_graph(n, seed, m=None):
    """A CSR graph of n rows over m columns (unsorted columns, fp32 weights in (0, 1]) that holds, where n allows: row 0 EMPTY, row 1
    a HUB of degree m - 1, row 2 of degree 1, row 3 with a SELF-LOOP, rows 4 and 5 with a column outside [0, m) on either side, and
    random rows of 0 .. 12 entries -> (rowptr, col, val)"""
    m = n if m is None else m
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        deg = int(rng.integers(0, 13))
        cols = rng.integers(0, m, deg).tolist()
        if i == 0 and n > 1:
            cols = []
        elif i == 1:
            cols = [j for j in range(m) if j != 1]
        elif i == 2:
            cols = [int(rng.integers(0, m))]
        elif i == 3:
            cols = cols[:3] + [3] + cols[3:]
        elif i == 4:
            cols = cols[:2] + [m + 5] + cols[2:]
        elif i == 5:
            cols = [-3] + cols
        rows.append(cols)
    if n == 1:
        rows = [[0, 7, 0, -1]]                                      # a self-loop twice and two columns that are no edges
    rowptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    col = np.array([c for r in rows for c in r], dtype=np.int64)
    val = rng.uniform(0.05, 1.0, len(col)).astype(np.float32)
    return rowptr, col, val


def special_labels(n, k, seed):
    rng = np.random.default_rng(seed)
    y = np.where(rng.uniform(size=n) < 0.4, rng.integers(0, k, n), -1).astype(np.int64)
    for i, v in zip(range(6, n, 11), itertools.cycle((k, 2 ** 40, -5, k - 1, 0))):
        y[i] = v
    return y


# ================================================================================================ sv_lp_normalize
@pytest.mark.parametrize("mode", [R.SYM, R.ROW])
@pytest.mark.parametrize("n", [1, 63, 300])
def test_normalize_degrees_bit_for_bit_and_values_within_one_ulp(n, mode):
    rowptr, col, val = special_graph(n, 9401 + n)
    sval, deg = normalize(rowptr, col, val, n, mode)
    ref_sval, ref_deg = R.csr_normalize(rowptr, col, val, n, mode)
    w = R.to_dense(rowptr, col, val, n)
    plain = w.sum(axis=1)
    edge = (col >= 0) & (col < n)
    rows_of = np.repeat(np.arange(n), np.diff(rowptr))
    # (duplicate columns are separate entries: each holds ITS weight over the row's degree)
    dd = ref_deg[rows_of[edge]] * (ref_deg[col[edge]] if mode == R.SYM else 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = np.where(dd == 0.0, 0.0, val[edge].astype(np.float64) / (np.sqrt(dd) if mode == R.SYM else dd))
    print("FIG normalize n=%d mode=%d: deg %.1f ulp64 of a plain sum, sval %.2f ulp32 of float64, bit-equal to the restatement: %s"
          % (n, mode, ulps64(deg, plain), ulps32(sval[edge], want), np.array_equal(sval, ref_sval)))
    assert np.array_equal(deg, ref_deg)
    assert ulps64(deg, plain) <= 1.0
    assert ulps32(sval[edge], want) <= 1.0 and (sval[~edge] == 0).all()
    if n > 1:
        assert deg[0] == 0.0                                        # the empty row
    # a repeat gives the same bits
    again = normalize(rowptr, col, val, n, mode)
    assert np.array_equal(again[0], sval) and np.array_equal(again[1], deg)


def test_normalize_is_exact_where_the_degrees_are_squares():
    """connectivity graphs K(4, 9) -- degrees 9 and 4, sqrt(36) = 6 --, a star K(1, 16) -- 16 and 1, sqrt(16) = 4 -- and K5 (degree 4)"""
    edges = [(a, 4 + b) for a in range(4) for b in range(9)] + [(13, 14 + b) for b in range(16)] \
        + [(30 + a, 30 + b) for a in range(5) for b in range(a + 1, 5)]
    n = 36                                                         # row 35 is isolated: degree 0
    w = np.zeros((n, n))
    for a, b in edges:
        w[a, b] = w[b, a] = 1.0
    rowptr, col, val = R.to_csr(w)
    sval, deg = normalize(rowptr, col, val, n, R.SYM)
    assert np.array_equal(deg, w.sum(axis=1)) and deg[35] == 0.0
    rows_of = np.repeat(np.arange(n), np.diff(rowptr))
    root = np.sqrt(deg[rows_of] * deg[col])
    assert np.array_equal(root, np.round(root)) and set(root.tolist()) == {4.0, 6.0}
    assert np.array_equal(sval, (1.0 / root).astype(np.float32))
    sval, _ = normalize(rowptr, col, val, n, R.ROW)
    assert np.array_equal(sval, (1.0 / deg[rows_of]).astype(np.float32))


def test_normalize_degree_zero_out_of_range_columns_and_an_empty_graph():
    # every entry of row 1 names a column outside the matrix: degree 0; row 0 reads row 1 (deg 0): 0, never a NaN
    rowptr, col, val = np.array([0, 2, 4, 5], dtype=np.int64), np.array([1, 2, 3, -1, 0], dtype=np.int64), np.array([1, 2, 3, 4, 5], dtype=np.float32)
    for mode in (R.SYM, R.ROW):
        sval, deg = normalize(rowptr, col, val, 3, mode)
        assert deg.tolist() == [3.0, 0.0, 5.0] and np.isfinite(sval).all()
        want = [0.0, 2 / np.sqrt(15.0), 0.0, 0.0, 5 / np.sqrt(15.0)] if mode == R.SYM else [1 / 3, 2 / 3, 0.0, 0.0, 1.0]
        assert np.array_equal(sval, np.array(want, dtype=np.float32))
    # N = 1 with no entry, col / val / sval NULL
    sval, deg = normalize(np.array([0, 0], dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float32), 1, R.SYM)
    assert deg.tolist() == [0.0] and sval.size == 0
    # a rowptr that points outside the arrays is clamped: nothing is read behind them
    sval, deg = normalize(np.array([-5, 2, 99, 7], dtype=np.int64), col, val, 3, R.ROW)
    assert deg.tolist() == [3.0, 5.0, 0.0]


# ================================================================================================ sv_lp_step
@pytest.mark.parametrize("k", [1, 2, 10, 16, 17, 64, 65, 257])
def test_step_is_the_restatement_bit_for_bit(k):
    for n in (1, 63, 64, 65, 300):
        rowptr, col, val = special_graph(n, 9411 + n)
        rng = np.random.default_rng(9413 + 7 * n + k)
        sval = rng.uniform(0.0, 1.0, len(col)).astype(np.float32)
        f_in = rng.uniform(0.0, 1.0, (n, k)).astype(np.float32)
        f_in[rng.uniform(size=(n, k)) < 0.3] = 0.0
        y = special_labels(n, k, 9415 + n)
        for variant in (R.SPREADING, R.PROPAGATION, R.PRODUCT):
            alpha = 0.2 if variant != R.SPREADING else (0.9, 0.2)[n % 2]
            label = None if variant == R.PRODUCT and n % 2 else y
            got = step(rowptr, col, sval, f_in, n, k, label, variant, alpha)
            want = R.csr_step(rowptr, col, sval, f_in, n, k, label, variant, alpha)
            assert np.array_equal(got, want), "n=%d k=%d variant=%d: %d elements differ, by at most %.3e" \
                % (n, k, variant, int((got != want).sum()), float(np.abs(got.astype(np.float64) - want).max()))
            if n > 1:
                if variant == R.PRODUCT:
                    assert not got[0].any()                         # the empty row
                # the same bits however the rows are cut into calls, and on a repeat
                cut = step(rowptr, col, sval, f_in, n, k, label, variant, alpha, cuts=sorted({1, n // 3, n - 1}))
                assert np.array_equal(cut, got)


def test_step_on_a_bipartite_graph_counts_labels_exactly():
    """PRODUCT with M != N: one-hot rows over a connectivity graph give the neighbours' label counts"""
    n, m, k = 70, 45, 19
    rowptr, col, _ = special_graph(n, 9421, m)
    cls = np.arange(m) % k
    got = step(rowptr, col, np.ones(len(col), dtype=np.float32), R.one_hot(cls, k), n, k, None, R.PRODUCT)
    want = np.zeros((n, k))
    for i in range(n):
        for q in range(rowptr[i], rowptr[i + 1]):
            if 0 <= col[q] < m:
                want[i, cls[col[q]]] += 1
    assert np.array_equal(got, want)


def test_a_nan_weight_reaches_only_the_rows_that_read_it():
    n, k = 130, 17
    rowptr, col, val = special_graph(n, 9423)
    rng = np.random.default_rng(9424)
    sval = rng.uniform(0.0, 1.0, len(col)).astype(np.float32)
    f_in = rng.uniform(0.1, 1.0, (n, k)).astype(np.float32)
    y = np.full(n, -1, dtype=np.int64)
    bad = sval.copy()
    hit = [7, 64, 129]
    for i in hit:
        assert rowptr[i + 1] > rowptr[i] and 0 <= col[rowptr[i]] < n
        bad[rowptr[i]] = np.nan
    for variant in (R.SPREADING, R.PROPAGATION, R.PRODUCT):
        clean = step(rowptr, col, sval, f_in, n, k, y, variant)
        got, stats = step(rowptr, col, bad, f_in, n, k, y, variant, stats=True)
        others = np.setdiff1d(np.arange(n), hit)
        assert np.isnan(got[hit]).all() and np.array_equal(got[others], clean[others])
        assert np.isnan(stats).all()
    # through sv_lp_normalize: a NaN weight makes its row's degree NaN, and with it the row and (SYM) the entries that name the row
    vbad = val.copy()
    vbad[rowptr[7]] = np.nan
    s_row, d_row = normalize(rowptr, col, vbad, n, R.ROW)
    rows_of = np.repeat(np.arange(n), np.diff(rowptr))
    edge = (col >= 0) & (col < n)
    assert np.isnan(d_row[7]) and np.isfinite(np.delete(d_row, 7)).all()
    assert np.array_equal(np.isnan(s_row), edge & (rows_of == 7))
    s_sym, _ = normalize(rowptr, col, vbad, n, R.SYM)
    assert np.array_equal(np.isnan(s_sym), edge & ((rows_of == 7) | (col == 7)))


def test_step_refuses_an_output_that_is_its_input():
    f = torch.zeros(8, 3, dtype=torch.float32, device=dev())
    rowptr, label = torch.zeros(9, dtype=torch.int64, device=dev()), torch.zeros(8, dtype=torch.int64, device=dev())
    rc = L.lib().sv_lp_step(p(f), 8, p(rowptr), None, None, 0, 8, 3, p(label), R.SPREADING, 0.2, 0.8, p(f), None, None, st())
    assert rc == -1 and b"aliases" in L.lib().sv_last_error()
    rc = L.lib().sv_lp_step(p(f), 8, p(rowptr), None, None, 0, 4, 3, p(label), R.SPREADING, 0.2, 0.8, p(f[4:]), None, None, st())
    assert rc == -1 and b"aliases" in L.lib().sv_last_error()
    torch.cuda.synchronize()
    assert not bool(f.any())


@pytest.mark.parametrize("n,k", [(1, 1), (65, 16), (300, 10), (300, 17), (4096, 10), (1030, 257)])
def test_statistics_match_float64_by_the_8x_rule(n, k):
    rowptr, col, val = special_graph(n, 9431 + n)
    rng = np.random.default_rng(9433 + k)
    sval = (rng.uniform(0.0, 1.0, len(col)) / 6.0).astype(np.float32)
    f_in = rng.uniform(0.0, 1.0, (n, k)).astype(np.float32)
    y = special_labels(n, k, 9435)
    for variant in (R.SPREADING, R.PROPAGATION):
        plain = step(rowptr, col, sval, f_in, n, k, y, variant)
        got, stats = step(rowptr, col, sval, f_in, n, k, y, variant, stats=True)
        assert np.array_equal(got, plain)                           # the statistics change no bit of f_out
        d64 = np.abs(got.astype(np.float64) - f_in.astype(np.float64))
        d32 = np.abs(got - f_in)                                    # the fp32 restatement of the same sums
        l1_32 = float(np.cumsum(d32.reshape(-1), dtype=np.float32)[-1])
        tol = 8.0 * max(abs(l1_32 - d64.sum()), R.half_ulp32(d64.sum()))
        print("FIG statistics n=%d k=%d variant=%d: delta_l1 %.6e err %.3e (allowance %.3e), delta_max %.6e"
              % (n, k, variant, stats[0], abs(stats[0] - d64.sum()), tol, stats[1]))
        assert abs(stats[0] - d64.sum()) <= tol
        assert stats[1] == d64.max()


# ================================================================================================ sv_lp_finish
@pytest.mark.parametrize("n,k", [(1, 1), (257, 2), (300, 10), (65, 257)])
def test_finish_normalises_within_one_ulp_and_counts_exactly(n, k):
    rng = np.random.default_rng(9441 + k)
    f = rng.uniform(0.0, 1.0, (n, k)).astype(np.float32)
    f[rng.uniform(size=(n, k)) < 0.3] = 0.0
    f[2::13] = 0.0
    nans = list(range(5, n, 29))
    for i in nans:
        f[i, i % k] = np.nan
    unreached = np.nonzero(~f.any(axis=1))[0]                        # (a NaN is not zero)
    got = finish(f)
    proba, pred, conf, counts = R.csr_finish(f)
    p64, pred64, _, counts64 = R.finish(f)
    ok = np.setdiff1d(np.arange(n), nans)
    print("FIG finish n=%d k=%d: proba %.2f ulp32 of float64, bit-equal to the restatement: %s"
          % (n, k, ulps32(got["proba"][ok], p64[ok]), np.array_equal(got["proba"], proba, equal_nan=True)))
    assert ulps32(got["proba"][ok], p64[ok]) <= 1.0 and np.isnan(got["proba"][nans]).all()
    assert np.array_equal(got["pred"], pred) and np.array_equal(got["pred"], pred64)
    assert (got["pred"][unreached] == -1).all() and (got["pred"][nans] == -1).all()
    decided = np.setdiff1d(ok, unreached)
    assert (got["pred"][decided] >= 0).all() and np.array_equal(got["conf"][decided], got["proba"][decided].max(axis=1))
    assert (got["conf"][np.setdiff1d(unreached, nans)] == 0).all()
    assert got["counts"].tolist() == list(counts) == list(counts64) == [len(decided), len(np.setdiff1d(unreached, nans))]
    # every subset of the outputs gives the same bits in the others
    names = ("proba", "pred", "conf", "counts")
    for r in range(1, 4):
        for want in itertools.combinations(names, r):
            part = finish(f, want=want)
            for name in want:
                assert np.array_equal(part[name], got[name], equal_nan=True), (want, name)


def test_finish_ties_go_to_the_smaller_index():
    n, k = 130, 66
    rng = np.random.default_rng(9443)
    half = np.floor(rng.uniform(0, 4, (n, k // 2)))
    f = np.concatenate([half, half], axis=1)                        # every class twice: exact ties, k / 2 apart
    got = finish(f)
    assert np.array_equal(got["pred"], np.where(half.sum(axis=1) == 0, -1, half.argmax(axis=1)))
    assert np.array_equal(got["proba"][:, :k // 2], got["proba"][:, k // 2:])


# ================================================================================================ LabelPropagator
def device_graph(case_, k_nn):
    """the k-NN graph of a blob case as THE DEVICE builds it, and the case's data"""
    x, cls, y, _ = case_
    rowptr, col, val = S.knn_graph(f32(x), None, k=k_nn, metric="euclid")
    return x, cls, y, rowptr, col, val


@pytest.mark.parametrize("variant", ["spreading", "propagation"])
def test_step_of_the_class_is_the_calls_by_hand_and_a_replayed_graph(variant):
    N, D, k_nn, K, per = CASES[1]
    x, cls, y, rowptr, col, val = device_graph(case(N, D, k_nn, K, per), k_nn)
    code = PG.VARIANTS[variant]
    lp = S.LabelPropagator(K, variant, alpha=0.2).prepare_graph(rowptr, col, val, i64(y))
    lp.step()
    lp.step()
    stats = lp.step().clone()
    # by hand
    hr, hc, hv = rowptr.cpu().numpy(), col.cpu().numpy(), val.cpu().numpy()
    sval, deg = normalize(hr, hc, hv, N, R.SYM if variant == "spreading" else R.ROW)
    assert np.array_equal(sval, lp.sval.cpu().numpy()) and np.array_equal(deg, lp.deg.cpu().numpy())
    f = R.one_hot(y, K).astype(np.float32)
    for _ in range(3):
        f, hand_stats = step(hr, hc, sval, f, N, K, y, code, 0.2, stats=True)
    assert np.array_equal(lp.f[lp.cur].cpu().numpy(), f) and np.array_equal(stats.cpu().numpy(), hand_stats)
    assert np.array_equal(f, R.csr_iterate(hr, hc, sval, y, N, K, code, 0.2, 3, 0.0)[0])
    # a graph of two steps, replayed; then on re-initialised (other) labels
    g = S.LabelPropagator(K, variant, alpha=0.2).prepare_graph(rowptr, col, val, i64(y))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            g.step()
            g.step()
    torch.cuda.current_stream().wait_stream(side)
    y2 = R.few_labels(cls, K, 2, 9451)
    for labels in (y, y2, y):
        g.reset(i64(labels))
        graph.replay()
        graph.replay()
        torch.cuda.synchronize()
        eager = S.LabelPropagator(K, variant, alpha=0.2).prepare_graph(rowptr, col, val, i64(labels))
        for _ in range(4):
            est = eager.step()
        assert g.cur == eager.cur == 0
        assert torch.equal(g.f[0], eager.f[0]) and torch.equal(g.f[1], eager.f[1]) and torch.equal(g.stats, est)


@pytest.mark.parametrize("variant", ["spreading", "propagation"])
@pytest.mark.parametrize("N,D,k_nn,K,per", CASES)
def test_fit_follows_the_restatement_from_the_devices_own_graph(N, D, k_nn, K, per, variant, monkeypatch):
    x, cls, y, _ = case(N, D, k_nn, K, per)
    code = PG.VARIANTS[variant]
    reads = []
    for name in ("cpu", "item", "tolist"):
        monkeypatch.setattr(torch.Tensor, name,
                            (lambda real: lambda self, *a, **k: (reads.append(1) if self.is_cuda else None, real(self, *a, **k))[1])(getattr(torch.Tensor, name)))
    dx, dy = f32(x), i64(y)
    lp = S.LabelPropagator(K, variant, alpha=0.2, k=k_nn, metric="euclid").fit(dx, None, dy, check_every=10)
    monkeypatch.undo()
    assert len(reads) == min(lp.n_iter_, lp.max_iter - 1) // 10 + 1, "fit reads delta_l1 once per check_every iterations, then the counts"
    # the float64 restatement on the graph the device built
    hr, hc, hv = lp.rowptr.cpu().numpy(), lp.col.cpu().numpy(), lp.val.cpu().numpy()
    w = R.to_dense(hr, hc, hv, N)
    assert np.array_equal(w, w.T) and not w.diagonal().any()
    s = R.normalize(w, R.SYM if variant == "spreading" else R.ROW)
    f64, n64, conv64, deltas = R.iterate(s, y, K, code, 0.2, lp.max_iter, 1e-3, 10)
    f32_, _, _, _ = R.iterate(s, y, K, code, 0.2, lp.max_iter, 1e-3, 10, np.float32)
    p64, pred64, _, counts64 = R.finish(f64)
    tol = R.allowance(R.finish(f32_)[0], p64)
    err = float(np.abs(host(lp.label_distributions_) - p64).max())
    decided = R.margin(p64) > 2.0 * tol
    acc = float((lp.transduction_.cpu().numpy() == cls)[y < 0].mean())
    print("FIG fit %s %s: n_iter %d (float64 %d), label_distributions_ err %.3e (allowance %.3e), undecided rows %d, delta %.3e "
          "(float64 %.3e), accuracy on the unlabelled rows %.3f" % ((N, D, k_nn, K, per), variant, lp.n_iter_, n64, err, tol, int((~decided).sum()),
                                                                   lp.delta_, deltas[n64 - 1], acc))
    assert (~decided).sum() <= 0.02 * N, "the reference leaves too many rows undecided: widen the blobs"
    assert lp.n_iter_ == n64 and lp.converged_ == conv64
    assert err <= tol
    assert np.array_equal(lp.transduction_.cpu().numpy()[decided], pred64[decided])
    assert lp.n_unreached_ == counts64[1] and np.abs(host(lp.label_distributions_).sum(axis=1) - (pred64 >= 0)).max() <= 4 * EPS32
    # ... and the emulation of the device's own arithmetic, bit for bit
    emu, n_emu, _, _ = R.csr_iterate(hr, hc, lp.sval.cpu().numpy(), y, N, K, code, 0.2, lp.max_iter, 1e-3, 10)
    assert n_emu == lp.n_iter_ and np.array_equal(lp.f[lp.cur].cpu().numpy(), emu)
    assert np.array_equal(lp.label_distributions_.cpu().numpy(), R.csr_finish(emu)[0])


def test_predict_on_the_fitted_rows_is_the_mean_over_their_neighbours():
    N, D, k_nn, K, per = CASES[0]
    x, cls, y, _ = case(N, D, k_nn, K, per)
    dx = f32(x)
    lp = S.LabelPropagator(K, "spreading", k=k_nn, metric="euclid").fit(dx, None, i64(y))
    proba, pred = lp.predict_proba(dx), lp.predict(dx)
    index = S.LatentIndex(D, "euclid")
    index.add(dx, None)
    idx = index.search(dx, None, k=k_nn)[1].cpu().numpy()
    assert (idx[:, 0] == np.arange(N)).all()                        # a fitted row finds itself first
    dist = host(lp.label_distributions_)
    mean = dist[idx].sum(axis=1)
    want = mean / np.where(mean.sum(axis=1) == 0, 1.0, mean.sum(axis=1))[:, None]
    err = float(np.abs(host(proba) - want).max())
    print("FIG predict %s: %.3e against the float64 neighbour mean (allowance %.3e)" % ((N, D, k_nn, K, per), err, 2 * EPS32))
    # three roundings of at most eps32 / 2 relative -- the product's output, the row sum of fp32 values, the quotient -- on values <= 1
    assert err <= 2 * EPS32
    decided = R.margin(want) > 4 * EPS32
    assert np.array_equal(pred.cpu().numpy()[decided], want.argmax(axis=1)[decided]) and decided.mean() >= 0.98
    assert torch.equal(pred, lp.predict(dx))
    # the state_dict round trip, through the host
    sd = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in lp.state_dict().items()}
    other = S.LabelPropagator(K).load_state_dict(sd, device=dev())
    assert torch.equal(other.predict_proba(dx), proba) and other.n_iter_ == lp.n_iter_ and torch.equal(other.transduction_, lp.transduction_)
    # a propagator fitted on a graph has no rows to search
    graph_only = S.LabelPropagator(K).prepare_graph(lp.rowptr, lp.col, lp.val, i64(y))
    for _ in range(lp.n_iter_):
        graph_only.step()
    graph_only.finish()
    assert torch.equal(graph_only.label_distributions_, lp.label_distributions_)
    with pytest.raises(ValueError, match="nothing to search"):
        graph_only.predict(dx)


def test_affinity_weights_and_the_posterior_metrics_build_a_symmetric_graph():
    N, D, k_nn, K, per = CASES[0]
    x, cls, y, _ = case(N, D, k_nn, K, per)
    rng = np.random.default_rng(9461)
    ls = f32(rng.normal(-1.0, 0.1, x.shape))
    for metric, weights in (("kl", "affinity"), ("w2", "connectivity"), ("euclid", "affinity")):
        rowptr, col, val = S.knn_graph(f32(x), None if metric == "euclid" else ls, k=k_nn, metric=metric, weights=weights)
        w = R.to_dense(rowptr.cpu().numpy(), col.cpu().numpy(), val.cpu().numpy(), N)
        assert np.array_equal(w, w.T) and not w.diagonal().any() and (w >= 0).all() and w.any(axis=1).all()
        lp = S.LabelPropagator(K, "propagation", k=k_nn, metric=metric, weights=weights, max_iter=40).fit(
            f32(x), None if metric == "euclid" else ls, i64(y))
        acc = float((lp.transduction_.cpu().numpy() == cls).mean())
        print("FIG knn_graph %s / %s: accuracy %.3f, unreached %d" % (metric, weights, acc, lp.n_unreached_))
        assert lp.n_iter_ == 40 and not lp.converged_
        assert acc > 1.0 / K + 0.1                                  # (three blobs whose centres lie 1.2 sqrt(2 D) = 3.8 noise units apart)


# ================================================================================================ the models
def batches_of(images, labels, B):
    return [(images[i:i + B], labels[i:i + B]) for i in range(0, images.shape[0], B)]


def carried_labels(mu_fit, mu_test):
    """labels the codes carry by construction: the side of the fit rows' median along their first principal direction"""
    c = mu_fit.mean(axis=0)
    direction = np.linalg.svd(mu_fit - c, full_matrices=False)[2][0]
    cut = np.median((mu_fit - c) @ direction)
    return ((mu_fit - c) @ direction > cut).astype(np.int64), ((mu_test - c) @ direction > cut).astype(np.int64)


def held_to_float64(res, y_true_all, n_fit, what):
    """a budget's figures against the float64 restatement on the propagator's OWN graph and labels"""
    lp = res["propagator"]
    n, K = lp.n, lp.k_classes
    y = lp.label.cpu().numpy()
    w = R.to_dense(lp.rowptr.cpu().numpy(), lp.col.cpu().numpy(), lp.val.cpu().numpy(), n)
    s = R.normalize(w, R.SYM if lp.variant == "spreading" else R.ROW)
    code = PG.VARIANTS[lp.variant]
    f64, n64, conv64, _ = R.iterate(s, y, K, code, lp.alpha, lp.max_iter, lp.tol, 10)
    f32_, _, _, _ = R.iterate(s, y, K, code, lp.alpha, lp.max_iter, lp.tol, 10, np.float32)
    p64, pred64, _, counts64 = R.finish(f64)
    tol = R.allowance(R.finish(f32_)[0], p64)
    err = float(np.abs(host(lp.label_distributions_) - p64).max())
    undecided = R.margin(p64) <= 2.0 * tol
    assert err <= tol and res["n_iter"] == n64 and res["converged"] == conv64 and res["n_unreached"] == counts64[1]
    hidden = (y[:n_fit] < 0)
    if hidden.any():
        ref = float((pred64[:n_fit] == y_true_all[:n_fit])[hidden].mean())
        assert abs(res["accuracy_unlabelled"] - ref) <= undecided[:n_fit][hidden].sum() / hidden.sum() + 1e-12, what
    if n > n_fit:                                                   # transductive: the test rows are rows of the graph
        ref = float((pred64[n_fit:] == y_true_all[n_fit:]).mean())
        assert abs(res["accuracy_test"] - ref) <= undecided[n_fit:].sum() / (n - n_fit) + 1e-12, what
    return err, tol


@pytest.mark.parametrize("kind", KR.EVAL_KINDS)
def test_evaluate_propagation_on_both_model_families(kind):
    from tests.test_cluster_gpu import eval_model
    model = eval_model(kind)
    gi, _, ti, _ = (t.to(dev()) for t in KR.eval_images(kind))
    mu_f, mu_t = S.encode_posterior(model, gi)[0], S.encode_posterior(model, ti)[0]
    yf, yt = carried_labels(host(mu_f), host(mu_t))
    gl, tl = i64(yf), i64(yt)
    y_all = np.concatenate([yf, yt])
    n_fit = KR.EVAL_GALLERY
    assert yf.mean() == 0.5
    chance = 0.5                                                    # the fit labels are balanced by construction (the median)
    args = dict(metric="euclid", k=10, variant="spreading", alpha=0.8, max_iter=60)
    for mode in ("transductive", "inductive"):
        res = S.evaluate_propagation(model, batches_of(gi, gl, 16), batches_of(ti, tl, 16), labels_per_class=[4, None], seed=3, mode=mode, **args)
        assert list(res) == [4, None]
        few, full = res[4], res[None]
        assert few["n_labelled"] == 8 and full["n_labelled"] == n_fit and np.isnan(full["accuracy_unlabelled"])
        assert few["propagator"].n == (n_fit + KR.EVAL_TEST if mode == "transductive" else n_fit)
        for m in res:
            err, tol = held_to_float64(res[m], y_all, n_fit, (kind, mode, m))
            print("FIG evaluate_propagation %s %s budget %s: labelled %d unlabelled %.3f test %.3f (chance %.3f) unreached %d n_iter %d; "
                  "label_distributions_ err %.3e (allowance %.3e)" % (kind, mode, m, res[m]["n_labelled"], res[m]["accuracy_unlabelled"],
                                                                     res[m]["accuracy_test"], chance, res[m]["n_unreached"], res[m]["n_iter"], err, tol))
        if mode == "inductive":                                     # predict, against the float64 neighbour mean of its own distributions
            lp = few["propagator"]
            idx = lp.index.search(mu_t, None, k=10)[1].cpu().numpy()
            mean = host(lp.label_distributions_)[idx].sum(axis=1)
            decided = R.margin(mean / np.where(mean.sum(axis=1) == 0, 1.0, mean.sum(axis=1))[:, None]) > 4 * EPS32
            ref = float((np.where(mean.sum(axis=1) == 0, -1, mean.argmax(axis=1)) == yt).mean())
            assert abs(few["accuracy_test"] - ref) <= (~decided).mean() + 1e-12
        # the codes carry the label along their direction of largest variance (27 % of the variance of the SHOT-VAE's codes, 9 % of the
        # smooth model's), so neighbours share it more often than not.  The float64 restatement on the CPU oracle's codes gives 0.82 /
        # 0.84 on the unlabelled fit rows and 0.79 .. 0.94 on the test rows for the SHOT-VAE, 0.58 / 0.59 and 0.60 .. 0.75 for the smooth
        # model: asserted to beat an even guess by 0.05
        assert few["accuracy_unlabelled"] >= chance + 0.05 and few["accuracy_test"] >= chance + 0.05 and full["accuracy_test"] >= chance + 0.05
        # re-batched: the images are regrouped before the encoder sees them and the rows are gathered before anything is fitted, so
        # the same rows give the same bits -- for both families
        other = S.evaluate_propagation(model, batches_of(gi, gl, 12), batches_of(ti, tl, 48), labels_per_class=[4, None], seed=3, mode=mode, **args)
        for m in (4, None):
            assert torch.equal(other[m]["propagator"].label_distributions_, res[m]["propagator"].label_distributions_)
            assert all(other[m][q] == res[m][q] or (np.isnan(other[m][q]) and np.isnan(res[m][q]))
                       for q in ("n_labelled", "accuracy_unlabelled", "accuracy_test", "n_unreached", "n_iter", "converged"))
    # without regrouping the SHOT-VAE's encoder may hand over other rows: each result is then held to its own reference
    loose = S.evaluate_propagation(model, batches_of(gi, gl, 12), batches_of(ti, tl, 48), labels_per_class=4, seed=3, chunk_rows=None, **args)
    held_to_float64(loose[4], y_all, n_fit, (kind, "loose"))
    if kind == "svhn":
        assert torch.equal(loose[4]["propagator"].label_distributions_, few_transductive(model, gi, gl, ti, tl, args))
    with pytest.raises(ValueError, match="test_batches"):
        S.evaluate_propagation(model, batches_of(gi, gl, 16), None, mode="inductive", **args)
    alone = S.evaluate_propagation(model, batches_of(gi, gl, 16), None, labels_per_class=4, seed=3, **args)
    assert np.isnan(alone[4]["accuracy_test"]) and alone[4]["propagator"].n == n_fit


def few_transductive(model, gi, gl, ti, tl, args):
    return S.evaluate_propagation(model, batches_of(gi, gl, 16), batches_of(ti, tl, 16), labels_per_class=4, seed=3,
                                  **args)[4]["propagator"].label_distributions_
