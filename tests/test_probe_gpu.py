"""Linear probes on a real MI355X: sv_probe_rows, sv_probe_accum and sv_probe_update through the C ABI against the float64 restatement
of tests/_probe_ref.py (pinned to torch.autograd and scikit-learn by tests/test_probe_cpu.py), then the Python layer
(shot_vae_amd.probe).

Integer-valued inputs are compared exactly.  Otherwise the allowances follow the project's 8x rule and are formed when the test runs,
never from a GPU result: R.allowance = 8 x the error of the fp32 numpy restatement of v, lse and loss against float64 on the case's own
inputs (never less than 8 half ulps of fp32 at the largest value).  A probability p = exp(v - lse) <= 1 inherits |dp| <= p (|dv| +
|dlse|) plus expf's own rounding, and a residual one more rounding of at most eps32 / 2: PROBA(tol) = 2 tol + 8 eps32, which also bounds
|sum_k p - 1|.  A prediction is compared with float64 on the rows whose float64 margin exceeds twice the allowance; on the separated
blobs that must be every row.  The partial states are compared bit for bit with the restatement's sums of the kernel's OWN resid in the
kernel's order, and with the float64 gradient by |dG| <= PROBA(tol) sum_i |x_id|.  Outputs carry guard rows.  The measured figures are
in DESIGN.md 4l."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import shot_vae_amd as S                                        # noqa: E402
from shot_vae_amd import _lib as L                              # noqa: E402
from shot_vae_amd import probe as PB                            # noqa: E402
from tests import _knn_ref as KR                                # noqa: E402
from tests import _probe_ref as R                               # noqa: E402

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


def i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev())


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def proba_tol(tol):
    return 2.0 * tol + 8.0 * EPS32


def model_for(N, K, D, seed, size=1.0):
    """-> (x, y, w, b) of fp32 values: overlapping rows, random weights of a size that keeps the scores in a few units"""
    x, y = R.overlapping(N, K, D, seed)
    rng = np.random.default_rng(seed + 1)
    f = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)          # noqa: E731
    return x, y, f(rng.normal(0, size / np.sqrt(D), (K, D))), f(rng.normal(0, 0.5, K))


def rows(x, w, b, y=None, cuts=None, want=("loss", "pred", "proba")):
    """sv_probe_rows over the rows cut at `cuts` -> (lse, loss, pred, proba) numpy; the guard rows stay as they were"""
    N, (K, D) = x.shape[0], w.shape
    dx, dw, db = f32(x), f32(w), f32(b)
    dy = i64(y) if y is not None else None
    lse = torch.full((N + GUARD,), -7.0, dtype=torch.float32, device=dev())
    loss = torch.full((N + GUARD,), -7.0, dtype=torch.float32, device=dev())
    a = torch.full((N + GUARD,), -7, dtype=torch.int64, device=dev())
    r = torch.full((N + GUARD, K), -7.0, dtype=torch.float32, device=dev())
    edges = [0] + list(cuts or []) + [N]
    for lo, hi in zip(edges[:-1], edges[1:]):
        L.call("sv_probe_rows", p(dx[lo:]), hi - lo, p(dw), p(db), K, D, p(dy[lo:]) if dy is not None else None, p(lse[lo:]),
               p(loss[lo:]) if "loss" in want else None, p(a[lo:]) if "pred" in want else None, p(r[lo:]) if "proba" in want else None, st())
    torch.cuda.synchronize()
    assert bool((lse[N:] == -7.0).all()) and bool((loss[N:] == -7.0).all()) and bool((a[N:] == -7).all()) and bool((r[N:] == -7.0).all()), \
        "sv_probe_rows wrote behind its outputs"
    for name, t in (("loss", loss), ("pred", a), ("proba", r)):
        if name not in want:
            assert bool((t == -7).all()), name
    return lse[:N].cpu().numpy(), loss[:N].cpu().numpy(), a[:N].cpu().numpy(), r[:N].cpu().numpy()


def accum(x, y, lse, loss, w, b, P, init=1, states=None, want_resid=True):
    """sv_probe_accum -> (sums float64 [P, stride], counts int64 [P, 2], resid or None, the device states)"""
    K, D = w.shape
    N = x.shape[0]
    stride = R.state_stride(K, D)
    if states is None:
        states = (torch.full((P + 1, stride), -7.0, dtype=torch.float64, device=dev()), torch.full((P + 1, 2), -7, dtype=torch.int64, device=dev()))
    resid = torch.full((N + GUARD, K), -7.0, dtype=torch.float32, device=dev()) if want_resid else None
    dx, dy, dl, do, dw, db = f32(x), i64(y), f32(lse), f32(loss), f32(w), f32(b)          # (held until the call has run)
    L.call("sv_probe_accum", p(dx), p(dy), p(dl), p(do), N, p(dw), p(db), K, D, p(states[0]), p(states[1]), P, init, p(resid), st())
    torch.cuda.synchronize()
    assert bool((states[0][P:] == -7.0).all()) and bool((states[1][P:] == -7).all()), "sv_probe_accum wrote behind its states"
    if want_resid:
        assert bool((resid[N:] == -7.0).all()), "sv_probe_accum wrote behind resid"
    return states[0][:P].cpu().numpy(), states[1][:P].cpu().numpy(), (resid[:N].cpu().numpy() if want_resid else None), states


def update(sums, counts, K, D, lam, inv_L, beta, theta, look):
    """sv_probe_update on fresh copies -> dict of numpy arrays (g: state 0 after the call)"""
    P = sums.shape[0]
    t = dict(sums=torch.from_numpy(sums.copy()).to(dev()), theta=torch.from_numpy(np.array(theta, dtype=np.float64)).to(dev()),
             look=torch.from_numpy(np.array(look, dtype=np.float64)).to(dev()), w=torch.full((K + GUARD, D), -7.0, dtype=torch.float32, device=dev()),
             b=torch.full((K + GUARD,), -7.0, dtype=torch.float32, device=dev()),
             stats=torch.full((4 + 2 * K + GUARD,), -7.0, dtype=torch.float64, device=dev()))
    dc = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int64)).to(dev())
    L.call("sv_probe_update", p(t["sums"]), p(dc), P, K, D, float(lam), float(inv_L), float(beta), p(t["theta"]),
           p(t["look"]), p(t["w"]), p(t["b"]), p(t["stats"]), st())
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in t.items()}
    assert (out["stats"][4 + 2 * K:] == -7.0).all()
    out["g"] = out["sums"][0, :-1].reshape(K, D + 1)
    out["stats"] = out["stats"][:4 + 2 * K]
    return out


def ulps64(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float((np.abs(a - b) / np.spacing(np.maximum(np.abs(b), np.finfo(np.float64).tiny))).max())


# ================================================================================================ sv_probe_rows
ROWS_SHAPES = [(1, 2, 1), (63, 16, 15), (64, 17, 16), (65, 64, 17), (130, 65, 33), (65, 257, 130)]


@pytest.mark.parametrize("N,K,D", ROWS_SHAPES)
def test_rows_match_float64_by_the_8x_rule(N, K, D):
    x, y, w, b = model_for(N, K, D, 9201)
    ref_l, ref_o, ref_a, ref_p = R.rows(x, w, b, y)
    tol = R.allowance(x, w, b, y)
    lse, loss, a, r = rows(x, w, b, y)
    err_l, err_o, err_p = float(np.abs(lse - ref_l).max()), float(np.abs(loss - ref_o).max()), float(np.abs(r - ref_p).max())
    err_s = float(np.abs(r.astype(np.float64).sum(axis=1) - 1.0).max())
    decided = R.margin(x, w, b) > 2.0 * tol
    print("FIG rows %s lse %.3e loss %.3e (%.3e) proba %.3e sum %.3e (%.3e) undecided %d"
          % ((N, K, D), err_l, err_o, tol, err_p, err_s, proba_tol(tol), int((~decided).sum())))
    assert err_l <= tol and err_o <= tol and err_p <= proba_tol(tol) and err_s <= proba_tol(tol)
    assert np.array_equal(a[decided], ref_a[decided]) and (a >= 0).all() and (a < K).all()
    assert (r[np.arange(N), a] == r.max(axis=1)).all()
    # rows cut into calls give the same bits
    if N > 2:
        l2, o2, a2, r2 = rows(x, w, b, y, cuts=[1, N // 2])
        assert np.array_equal(l2, lse) and np.array_equal(o2, loss) and np.array_equal(a2, a) and np.array_equal(r2, r)


def test_every_subset_of_the_optional_outputs_gives_the_same_bits():
    x, y, w, b = model_for(70, 19, 21, 9203)
    full = dict(zip(("lse", "loss", "pred", "proba"), rows(x, w, b, y)))
    for k in range(3):
        for want in itertools.combinations(("loss", "pred", "proba"), k):
            got = dict(zip(("lse", "loss", "pred", "proba"), rows(x, w, b, y, want=want)))
            for name in ("lse",) + want:
                assert np.array_equal(got[name], full[name]), (want, name)
    # without labels: lse, pred and proba as before
    got = rows(x, w, b, None, want=("pred", "proba"))
    assert np.array_equal(got[0], full["lse"]) and np.array_equal(got[2], full["pred"]) and np.array_equal(got[3], full["proba"])


@pytest.mark.parametrize("N,K,D", [(130, 66, 1), (65, 10, 17), (63, 258, 16)])
def test_pred_is_the_first_maximum_on_integer_rows_with_tied_classes(N, K, D):
    rng = np.random.default_rng(9205)
    half = np.floor(rng.uniform(-2, 3, (K // 2, D)))
    w = np.concatenate([half, half])                         # every class twice: exact ties, K / 2 apart
    b = np.concatenate([np.arange(K // 2) % 3, np.arange(K // 2) % 3]).astype(np.float64)
    x = np.floor(rng.uniform(-2, 3, (N, D)))
    v = R.scores(x, w, b)
    ref_a = R.rows(x, w, b)[2]
    assert ((v == v.max(axis=1, keepdims=True)).sum(axis=1) > 1).all() and (ref_a < K // 2).all()
    lse, _, a, r = rows(x, w, b, None, want=("pred", "proba"))
    assert np.array_equal(a, ref_a) and np.array_equal(r[:, :K // 2], r[:, K // 2:])


def test_rules_of_special_rows_and_labels():
    N, K, D = 70, 5, 19
    x, y, w, b = model_for(N, K, D, 9207)
    x[3, 18], x[64, 0], x[65, 7] = np.nan, np.inf, -np.inf
    w[2, 0] = 0.0                                            # inf * 0 under class 2: still a NaN row
    y[10], y[11], y[12] = -1, K, 2 ** 40
    lse, loss, a, r = rows(x, w, b, y)
    bad = [3, 64, 65]
    ok = np.setdiff1d(np.arange(N), bad)
    assert np.isnan(lse[bad]).all() and np.isnan(loss[bad]).all() and (a[bad] == -1).all() and np.isnan(r[bad]).all()
    assert np.isfinite(lse[ok]).all() and np.isfinite(r[ok]).all() and (a[ok] >= 0).all()
    assert np.isnan(loss[[10, 11, 12]]).all() and np.isfinite(loss[np.setdiff1d(ok, [10, 11, 12])]).all()
    # the neighbours of the special rows are the rows they are without them
    clean = x.copy()
    clean[bad] = 0.0
    l2, o2, a2, r2 = rows(clean, w, b, y)
    assert np.array_equal(l2[ok], lse[ok]) and np.array_equal(o2[ok], loss[ok], equal_nan=True) and np.array_equal(a2[ok], a[ok])
    assert np.array_equal(r2[ok], r[ok])
    tol = R.allowance(x[ok], w, b, y[ok])
    ref = R.rows(x, w, b, y)
    assert np.abs(lse[ok] - ref[0][ok]).max() <= tol and np.nanmax(np.abs(loss[ok] - ref[1][ok])) <= tol


def test_rows_leave_no_row_of_separated_blobs_undecided():
    for N, K, D in ((193, 3, 5), (130, 10, 128), (193, 65, 130)):
        x, cen, which = R.blobs(N, K, D, 9209)
        w = (cen / 4.0).astype(np.float32).astype(np.float64)           # the nearest centre wins: v = c.x / 4 - |c|^2 / 8
        b = (-(w * w).sum(axis=1) * 2.0).astype(np.float32).astype(np.float64)
        tol = R.allowance(x, w, b, which)
        margin = R.margin(x, w, b)
        assert (margin > 2.0 * tol).all(), "the reference leaves a row undecided"
        lse, loss, a, _ = rows(x, w, b, which, want=("loss", "pred"))
        ref = R.rows(x, w, b, which)
        print("FIG blobs %s lse %.3e loss %.3e (%.3e) least margin %.3e" % ((N, K, D), np.abs(lse - ref[0]).max(), np.abs(loss - ref[1]).max(), tol,
                                                                           margin.min()))
        assert np.array_equal(a, which) and np.array_equal(a, ref[2])


# ================================================================================================ sv_probe_accum
def test_resid_is_proba_minus_the_one_hot_rounded_once():
    for N, K, D in ((70, 5, 19), (66, 70, 33)):
        x, y, w, b = model_for(N, K, D, 9211)
        y[4], y[65] = -1, K
        x[9, 0] = np.nan
        lse, loss, _, proba = rows(x, w, b, y)
        _, counts, resid, _ = accum(x, y, lse, loss, w, b, 1)
        hot = np.zeros((N, K), dtype=np.float32)
        used = R.used_rows(x, y, K)
        hot[np.nonzero(used)[0], y[used]] = 1
        want = np.where(used[:, None], proba - hot, np.float32(0)).astype(np.float32)
        assert np.array_equal(resid, want) and counts.tolist() == [[N - 3, 3]]


ACCUM_CASES = [(K, D, P, N) for (K, D) in ((5, 19), (70, 33)) for P in (1, 3, 64) for N in sorted({64, 65, 64 * P, 64 * P + 1})]


@pytest.mark.parametrize("K,D,P,N", ACCUM_CASES)
def test_accum_states_hold_the_kernels_own_sums_bit_for_bit(K, D, P, N):
    x, y, w, b = model_for(N, K, D, 9213)
    y[::7] = -1                                              # skipped rows interleaved
    y[N // 2] = K
    x[N - 1, D - 1] = np.inf
    lse, loss, _, _ = rows(x, w, b, y, want=("loss",))
    sums, counts, resid, states = accum(x, y, lse, loss, w, b, P)
    xz = np.where(np.isfinite(x), x, 0.0)
    want, wc = R.accum(xz, resid, y, lse, np.nan_to_num(loss), P)
    used = R.used_rows(x, y, K)
    assert np.array_equal(counts, wc) and int(counts[:, 0].sum()) == int(used.sum()) and int(counts.sum()) == N
    print("FIG accum %s against its own resid: %.1f ulp of double" % ((N, K, D, P), ulps64(sums, want)))
    assert np.array_equal(sums, want)
    # a repeat gives the same bits, with and without resid
    assert np.array_equal(accum(x, y, lse, loss, w, b, P, want_resid=False)[0], sums)
    # init = 0 continues: cut at a multiple of 64 P, the states hold the bits of the one call
    cut = 64 * P * max(1, (N // (64 * P)) // 2) if P > 1 else 64
    if cut < N:
        _, _, _, part = accum(x[:cut], y[:cut], lse[:cut], loss[:cut], w, b, P)
        s2, c2, _, _ = accum(x[cut:], y[cut:], lse[cut:], loss[cut:], w, b, P, init=0, states=part)
        assert np.array_equal(s2, sums) and np.array_equal(c2, counts)
    # ... and the same rows again double every count
    _, c4, _, _ = accum(x, y, lse, loss, w, b, P, init=0, states=states)
    assert np.array_equal(c4, 2 * counts)


def test_accum_matches_the_float64_gradient_by_the_8x_rule():
    N, K, D, P = 4096, 10, 16, 64
    x, y, w, b = model_for(N, K, D, 9215)
    y[5] = -1
    lse, loss, _, _ = rows(x, w, b, y, want=("loss",))
    sums, counts, _, _ = accum(x, y, lse, loss, w, b, P, want_resid=False)
    used = R.used_rows(x, y, K)
    assert counts.sum(axis=0).tolist() == [N - 1, 1]
    tol = proba_tol(R.allowance(x[used], w, b, y[used]))
    got = R.merge(sums)
    ref = R.gradient(x, y, R.pack(w, b), 0.0) * float(used.sum())
    ax = np.abs(x[used])
    bound = np.concatenate([[float(used.sum())], ax.sum(axis=0)]) * tol
    err = np.abs(got[:-1].reshape(K, D + 1) - ref)
    ref_loss = R.rows(x[used], w, b, y[used])[1].sum()
    print("FIG accum %s against float64: intercept %.3e (%.3e) weights %.3e (%.3e) loss sum %.3e (%.3e)"
          % ((N, K, D, P), err[:, 0].max(), bound[0], err[:, 1:].max(), bound[1:].min(), abs(got[-1] - ref_loss), used.sum() * tol))
    assert (err <= bound[None, :]).all() and abs(got[-1] - ref_loss) <= used.sum() * tol


# ================================================================================================ sv_probe_update
@pytest.mark.parametrize("N,K,D,P", [(200, 3, 5, 1), (453, 17, 33, 3), (300, 5, 300, 2), (4096, 10, 16, 64)])
def test_update_is_the_double_restatement(N, K, D, P):
    x, y, w, b = model_for(N, K, D, 9217)
    y[3] = -1
    lse, loss, _, _ = rows(x, w, b, y, want=("loss",))
    sums, counts, _, _ = accum(x, y, lse, loss, w, b, P, want_resid=False)
    rng = np.random.default_rng(9218)
    look = R.pack(w, b) + 1e-3 * rng.normal(size=(K, D + 1))
    theta = look + 1e-2 * rng.normal(size=(K, D + 1))
    lam, inv_L, beta = 1.0 / N, 0.37, 0.8
    got = update(sums, counts, K, D, lam, inv_L, beta, theta, look)
    g, tn, ln, w32, b32, stats = R.update(sums, counts, K, D, lam, inv_L, beta, theta, look)
    figs = (ulps64(got["g"], g), ulps64(got["theta"], tn), ulps64(got["look"], ln), ulps64(got["stats"][:2], stats[:2]),
            ulps64(got["stats"][4:], stats[4:]))
    print("FIG update %s ulp of double: g %.1f theta %.1f look %.1f objective / max |g| %.1f partials %.1f" % (((N, K, D, P),) + figs))
    # every operation is restated in its order: the allowance is the one rounding a fused or re-associated operation could differ by
    assert max(figs) <= 2.0
    assert got["stats"][2] == N - 1 and got["stats"][3] == 1
    # w, b: look rounded once; nothing behind them
    assert np.array_equal(got["w"][:K], got["look"][:, 1:].astype(np.float32)) and np.array_equal(got["b"][:K], got["look"][:, 0].astype(np.float32))
    assert (got["w"][K:] == -7.0).all() and (got["b"][K:] == -7.0).all()


def test_update_without_a_used_row_changes_nothing():
    K, D, P = 3, 4, 2
    rng = np.random.default_rng(9219)
    theta, look = rng.normal(size=(K, D + 1)), rng.normal(size=(K, D + 1))
    got = update(np.zeros((P, R.state_stride(K, D))), np.array([[0, 5], [0, 2]], dtype=np.int64), K, D, 0.1, 0.5, 0.3, theta, look)
    assert np.array_equal(got["theta"], theta) and np.array_equal(got["look"], look)
    assert (got["w"] == -7.0).all() and (got["b"] == -7.0).all()
    assert np.isnan(got["stats"][:2]).all() and got["stats"][2:4].tolist() == [0.0, 7.0]


# ================================================================================================ LinearProbe
def started(K, D, lam, lip, beta):
    return S.LinearProbe(K, D, standardize=False).start(dev(), lam, lip, beta)


def test_step_is_the_three_calls_by_hand_and_a_replayed_graph():
    N, K, D = 700, 5, 19
    x, y = R.overlapping(N, K, D, 9221)
    y[::9] = -1
    rows_, _, _, lam, lip, beta = R.constants(x, y, K, 1.0)
    lp = started(K, D, lam, lip, beta)
    dx, dy = f32(rows_), i64(y)
    lp.step(dx, dy)
    stats = lp.step(dx, dy).clone()                          # the second step starts from a point that is not 0
    # by hand
    hand = started(K, D, lam, lip, beta)
    hand.step(dx, dy)
    w0, b0, th0, lk0 = host(hand.w), host(hand.b), host(hand.theta), host(hand.look)
    lse, loss, _, _ = rows(rows_, w0, b0, y, want=("loss",))
    P = PB._partials(K, D, N)
    sums, counts, _, _ = accum(rows_, y, lse, loss, w0, b0, P, want_resid=False)
    got = update(sums, counts, K, D, lam, 1.0 / lip, beta, th0, lk0)
    assert np.array_equal(host(lp.theta), got["theta"]) and np.array_equal(host(lp.look), got["look"])
    assert np.array_equal(host(lp.w), got["w"][:K]) and np.array_equal(host(lp.b), got["b"][:K]) and np.array_equal(host(stats), got["stats"])
    # a graph captured on one set of rows, replayed on another
    bx, by = dx.clone(), dy.clone()
    g2 = started(K, D, lam, lip, beta)
    g2.step(bx, by)                                          # (allocates the workspace)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            g2.step(bx, by)
    torch.cuda.current_stream().wait_stream(side)
    x2, y2 = R.overlapping(N, K, D, 9223)
    r2 = ((x2 - x2.mean(axis=0)) / x2.std(axis=0)).astype(np.float32)
    for rows2, lab in ((r2, y2), (rows_, y)):
        bx.copy_(f32(rows2))
        by.copy_(i64(lab))
        for t in (g2.theta, g2.look, g2.w, g2.b):
            t.zero_()
        graph.replay()
        graph.replay()
        torch.cuda.synchronize()
        eager = started(K, D, lam, lip, beta)
        eager.step(f32(rows2), i64(lab))
        est = eager.step(f32(rows2), i64(lab))
        assert torch.equal(g2.theta, eager.theta) and torch.equal(g2.look, eager.look) and torch.equal(g2.w, eager.w) and torch.equal(g2.b, eager.b)
        assert torch.equal(g2.stats, est)
    assert torch.equal(g2.look, lp.look)


@pytest.mark.parametrize("N,K,D,iters", [(300, 3, 5, 400), (512, 10, 16, 1500)])
def test_fit_follows_the_restatement_from_the_same_constants(N, K, D, iters, monkeypatch):
    x, y = R.overlapping(N, K, D, 9107)
    y[7] = -1
    rows_, mean, scale, lam, lip, beta = R.constants(x, y, K, 1.0)
    # the solver alone, from the restatement's own rows and constants
    solver = started(K, D, lam, lip, beta)
    dx, dy = f32(rows_), i64(y)
    for _ in range(iters):
        solver.step(dx, dy)
    _, look64, _ = R.nesterov(rows_, y, K, lam, lip, beta, iters)
    _, look32, _ = R.nesterov(rows_, y, K, lam, lip, beta, iters, np.float32)
    tol = 8.0 * max(float(np.abs(look32 - look64).max()), R.half_ulp32(look64))
    err = float(np.abs(host(solver.look) - look64).max())
    gmax = float(np.abs(R.gradient(rows_, y, R.pack(host(solver.w), host(solver.b)), lam)).max())
    print("FIG fit %s after %d iterations: look err %.3e (%.3e), float64 max |g| at the fitted parameters %.3e, the device's own %.3e"
          % ((N, K, D), iters, err, tol, gmax, float(solver.stats[1])))
    assert err <= tol
    assert gmax < 1e-6
    assert float(solver.stats[1]) < 1e-6 and float(solver.stats[2]) == N - 1 and float(solver.stats[3]) == 1
    # fit(): its preparation in torch gives the restatement's constants, with ONE read from the device
    reads = []
    for name in ("cpu", "item", "tolist"):
        monkeypatch.setattr(torch.Tensor, name,
                            (lambda real: lambda self, *a, **k: (reads.append(1) if self.is_cuda else None, real(self, *a, **k))[1])(getattr(torch.Tensor, name)))
    lp = S.LinearProbe(K, D, C=1.0).fit(f32(x), i64(y), max_iter=iters, tol=None)
    monkeypatch.undo()
    assert len(reads) == 1, "fit(tol=None) reads the Gram matrix once and nothing else"
    assert lp.n_iter_ == iters and lp.converged_ is False
    assert abs(lp.lam - lam) <= 1e-15 * lam and abs(lp.lipschitz - lip) <= 1e-9 * lip and abs(lp.beta - beta) <= 1e-9
    assert np.abs(host(lp.mean) - mean).max() <= 1e-12 and np.abs(host(lp.scale) - scale).max() <= 1e-12
    assert float(np.abs(R.gradient(rows_, y, R.pack(host(lp.w), host(lp.b)), lam)).max()) < 1e-6
    # the stopping rule on the device's own gradient: converged well before max_iter, at a checked iteration
    early = S.LinearProbe(K, D, C=1.0).fit(f32(x), i64(y), max_iter=iters, tol=1e-4, check_every=10)
    assert early.converged_ and early.n_iter_ % 10 == 0 and early.n_iter_ < iters and float(early.stats[1]) < 1e-4


def test_fit_on_separated_blobs_and_the_views_of_the_fitted_model():
    N, K, D = 400, 4, 6
    x, cen, which = R.blobs(N, K, D, 9225, spread=0.5)
    y = which.copy()
    y[::5] = -1                                              # unlabelled rows: skipped, still predicted
    dx, dy = f32(x), i64(y)
    lp = S.LinearProbe(K, D).fit(dx, dy, max_iter=300, tol=1e-4)
    raw = S.LinearProbe(K, D, standardize=False).fit(dx, dy, max_iter=500, tol=None)
    pred = lp.predict(dx).cpu().numpy()
    assert np.array_equal(pred, which) and np.array_equal(raw.predict(dx).cpu().numpy(), which)
    assert float(lp.score(dx, dy)) == 1.0 and float(lp.score(dx, i64(which))) == 1.0
    proba = host(lp.predict_proba(dx))
    assert np.abs(proba.sum(axis=1) - 1.0).max() <= 1e-5 and np.array_equal(proba.argmax(axis=1), pred)
    # the rows the scans read, and the float64 restatement on them
    xs = ((x - host(lp.mean)) / host(lp.scale)).astype(np.float32).astype(np.float64)
    w, b = host(lp.w), host(lp.b)
    tol = R.allowance(xs, w, b, which)
    ref = R.rows(xs, w, b, y)
    used = y >= 0
    assert abs(float(lp.log_loss(dx, dy)) - ref[1][used].mean()) <= tol
    assert (R.margin(xs, w, b) > 2.0 * tol).all(), "the reference leaves a row undecided"
    # coef_ / intercept_ in raw coordinates reproduce decision_function
    logits = host(lp.decision_function(dx))
    raw_v = x @ host(lp.coef_).T + host(lp.intercept_)
    assert np.abs(logits - R.scores(xs, w, b)).max() <= R.half_ulp32(logits) * 2
    # (the scans' rows are rounded to fp32: each term w_d xs_d moves by at most eps32 / 2 of itself; then the logit's own rounding)
    assert (np.abs(raw_v - logits) <= 0.5 * EPS32 * (np.abs(xs) @ np.abs(w).T) + R.half_ulp32(logits) + 1e-12).all()
    # through calibration.row_stats: the predictions, and the loss within one allowance on each side
    rs = S.row_stats(lp.decision_function(dx), i64(which))
    assert np.array_equal(rs.pred.cpu().numpy(), pred)
    per_row = rows(xs, w, b, which, want=("loss",))[1]
    assert np.abs(host(rs.nll) - per_row).max() <= 2.0 * tol
    # the state_dict round trip
    sd = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in lp.state_dict().items()}
    other = S.LinearProbe(K, D).load_state_dict(sd, device=dev())
    assert torch.equal(other.predict_proba(dx), lp.predict_proba(dx)) and torch.equal(other.coef_, lp.coef_)
    assert other.converged_ == lp.converged_ and other.n_iter_ == lp.n_iter_


# ================================================================================================ the models
def batches_of(images, labels, B):
    return [(images[i:i + B], labels[i:i + B]) for i in range(0, images.shape[0], B)]


def carried_labels(mu_fit, mu_test):
    """labels the codes carry by construction: the side of the fit rows' median along their first principal direction"""
    c = mu_fit.mean(axis=0)
    direction = np.linalg.svd(mu_fit - c, full_matrices=False)[2][0]
    cut = np.median((mu_fit - c) @ direction)
    return ((mu_fit - c) @ direction > cut).astype(np.int64), ((mu_test - c) @ direction > cut).astype(np.int64)


def held_to_float64(res, x_test, y_test):
    """a budget's test figures against the float64 restatement at the probe's OWN parameters on the rows it was given"""
    lp = res["probe"]
    xs = ((host(x_test) - host(lp.mean)) / host(lp.scale)).astype(np.float32).astype(np.float64)
    w, b = host(lp.w), host(lp.b)
    tol = R.allowance(xs, w, b, y_test)
    ref = R.rows(xs, w, b, y_test)
    undecided = int((R.margin(xs, w, b) <= 2.0 * tol).sum())
    assert abs(res["nll_test"] - ref[1].mean()) <= tol
    assert abs(res["accuracy_test"] - (ref[2] == y_test).mean()) <= undecided / len(y_test) + 1e-12
    return tol


@pytest.mark.parametrize("kind", KR.EVAL_KINDS)
def test_evaluate_probe_on_both_model_families(kind):
    from tests.test_cluster_gpu import eval_model
    model = eval_model(kind)
    gi, _, ti, _ = (t.to(dev()) for t in KR.eval_images(kind))
    mu_f, mu_t = S.encode_posterior(model, gi)[0], S.encode_posterior(model, ti)[0]
    yf, yt = carried_labels(host(mu_f), host(mu_t))
    gl, tl = i64(yf), i64(yt)
    args = dict(max_iter=200, tol=None, C=1.0)
    res = S.evaluate_probe(model, batches_of(gi, gl, 16), batches_of(ti, tl, 16), labels_per_class=[4, None, 1000], seed=3, **args)
    assert list(res) == [4, None, 1000]
    full, few = res[None], res[4]
    assert full["n_labelled"] == KR.EVAL_GALLERY and few["n_labelled"] == 8 and full["n_iter"] == 200 and full["converged"] is False
    for m in res:
        tol = held_to_float64(res[m], mu_t, yt)
        print("FIG evaluate_probe %s budget %s: labelled %d fit %.3f test %.3f nll %.4f (allowance %.1e)"
              % (kind, m, res[m]["n_labelled"], res[m]["accuracy_fit"], res[m]["accuracy_test"], res[m]["nll_test"], tol))
    # the codes carry the label along their direction of largest variance.  A degenerate probe -- one answer for every row -- reaches at
    # most the larger class's share of the test rows; the float64 restatement on the CPU oracle's codes gives 1.0 on the fit rows and
    # 0.96 / 0.85 on the test rows (larger class: 0.63 / 0.71)
    assert full["accuracy_fit"] >= 0.9 and full["accuracy_test"] > max(yt.mean(), 1.0 - yt.mean())
    assert set(full["probe"].predict(mu_t).cpu().tolist()) == {0, 1}
    # a budget of all labels is labels_per_class=None
    assert torch.equal(res[1000]["probe"].look, full["probe"].look)
    assert all(res[1000][q] == full[q] for q in ("n_labelled", "accuracy_fit", "accuracy_test", "nll_test"))
    # re-batched: the rows are gathered before anything is fitted, so the same rows give the same bits.  (An encoder whose own bits
    # depend on its batch size hands over other rows: then each result is held to its own reference.)
    other = S.evaluate_probe(model, batches_of(gi, gl, 12), batches_of(ti, tl, 48), labels_per_class=[4, None], seed=3, **args)
    again = torch.cat([S.encode_posterior(model, x)[0] for x, _ in batches_of(gi, gl, 12)])
    same = torch.equal(again, mu_f) and torch.equal(torch.cat([S.encode_posterior(model, x)[0] for x, _ in batches_of(ti, tl, 16)]), mu_t)
    print("FIG evaluate_probe %s: the encoder's rows %s on the batch size" % (kind, "do not depend" if same else "DEPEND"))
    if kind == "svhn":
        assert same
    if same:
        for m in (4, None):
            assert torch.equal(other[m]["probe"].look, res[m]["probe"].look)
            assert all(other[m][q] == res[m][q] for q in ("n_labelled", "accuracy_fit", "accuracy_test", "nll_test"))
    else:
        for m in (4, None):
            held_to_float64(other[m], S.encode_posterior(model, ti)[0], yt)
    twice = S.evaluate_probe(model, batches_of(gi, gl, 16), batches_of(ti, tl, 16), labels_per_class=4, seed=3, **args)
    assert torch.equal(twice[4]["probe"].look, few["probe"].look) and twice[4]["accuracy_test"] == few["accuracy_test"]
    if kind != "svhn":
        feat = S.evaluate_probe(model, batches_of(gi, gl, 16), batches_of(ti, tl, 16), space="features", **args)
        assert feat[None]["probe"].dim == model.features(gi[:2]).shape[1] and 0.0 <= feat[None]["accuracy_test"] <= 1.0
    else:
        with pytest.raises(ValueError, match="features"):
            S.evaluate_probe(model, batches_of(gi, gl, 16), batches_of(ti, tl, 16), space="features")
