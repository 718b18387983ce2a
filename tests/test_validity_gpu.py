"""Internal cluster validity on a real MI355X: sv_sil_scan, sv_sil_finish and sv_cluster_spread through the C ABI -- `part` bit-equal to
the restatement of tests/_validity_ref.py that walks the kernel's order (columns, tiles of a segment, clusters of a state, the
butterfly), s / a / b bit-equal across P, query cuts and repeats, against float64 by the 8x rule, exact on integer data, the special
cases (one cluster, unknown labels, NaN rows, a seg beyond the gallery) -- then the Python layer (shot_vae_amd.validity).

Allowances are derived, never taken from a GPU result: R.allowance is 8 x the error of the fp32 restatement (the kernel's fp32 pair
values and fp32 roots, float64 sums) against float64; R.indices_allowance does the same for the two centroid indices.  Outputs carry
guard elements.  The bit-equality under SV_SIL_EUCLID holds only if the device's sqrtf is the correctly rounded fp32 root (numpy's
float32 sqrt): these tests are that check.

Measured on an MI355X (the FIG lines this file prints; DESIGN.md 4p has the table): `part` is bit-equal under both metrics at every
shape and P -- the device's sqrtf is numpy's float32 sqrt --; against float64 the kernel's error equals the fp32 restatement's in every
case: s 2.0e-8 .. 1.7e-7 (allowances 1.6e-7 .. 1.4e-6; exactly 0 at (2, 2, 1)), a and b 3.7e-9 .. 1.2e-6 under euclid and up to 5.5e-5
under sqeuclid (4.4e-4); silhouette_samples 193 x 17, K = 65: 1.3e-7 (1.0e-6); validity_indices 257 x 128, K = 10: silhouette
0.4009543241 (float64 0.4009543244), calinski_harabasz 62.96089854 (62.96089867, allowance 1.1e-6), davies_bouldin 0.9482791584
(0.9482791562, 1.7e-8); evaluate_validity on the true classes of the untrained models: silhouette -0.084 (wideresnet-10-1) and
-0.064 (svhn) in mu, -0.085 / -0.054 in w2."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import shot_vae_amd as S                                        # noqa: E402
from shot_vae_amd import _lib as L                              # noqa: E402
from shot_vae_amd import validity as V                          # noqa: E402
from tests import _knn_ref as KR                                # noqa: E402
from tests import _validity_ref as R                            # noqa: E402

GUARD = 5
SENTINEL = -7.0
ISENT = -77


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


def guarded(n, dtype=torch.float64):
    fill = ISENT if dtype == torch.int64 else SENTINEL
    return torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev())


def unguard(buf, n, what):
    fill = ISENT if buf.dtype == torch.int64 else SENTINEL
    assert bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all()), "%s was written beside its end" % what
    return buf[GUARD:GUARD + n].cpu().numpy()


def same(a, b):
    """equal in every bit; a NaN equals a NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    view = np.int64 if a.dtype == np.float64 else np.int32
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(view), b[~nb].view(view)))


def raw_scan(metric, dq, dql, dg, dseg, N, K, P):
    """one sv_sil_scan on device tensors -> (part_a, part_b) float64 numpy [P, Q]"""
    Q, D = dq.shape
    ba, bb = guarded(P * Q), guarded(P * Q)
    L.call("sv_sil_scan", metric, p(dq), p(dql), Q, p(dg), p(dseg), N, K, D, P, p(ba[GUARD:]), p(bb[GUARD:]), st())
    torch.cuda.synchronize()
    return unguard(ba, P * Q, "part_a").reshape(P, Q), unguard(bb, P * Q, "part_b").reshape(P, Q)


def raw_finish(pa, pb, ql, seg, K, N, want_a=True, want_b=True, want_cluster=True):
    """sv_sil_finish -> dict of numpy arrays: s, and a, b, cluster_sum, cluster_cnt, skipped where asked for"""
    P, Q = pa.shape
    bs, ba, bb = guarded(Q), guarded(Q), guarded(Q)
    bsum, bcnt, bskip = guarded(K), guarded(K, torch.int64), guarded(1, torch.int64)
    dpa, dpb, dql, dseg = f64(pa), f64(pb), i64(ql), i64(seg)      # (held: a temporary's memory would be handed to the next one)
    L.call("sv_sil_finish", p(dpa), p(dpb), P, Q, p(dql), p(dseg), K, N, p(bs[GUARD:]), p(ba[GUARD:]) if want_a else None,
           p(bb[GUARD:]) if want_b else None, p(bsum[GUARD:]) if want_cluster else None, p(bcnt[GUARD:]) if want_cluster else None,
           p(bskip[GUARD:]) if want_cluster else None, st())
    torch.cuda.synchronize()
    out = dict(s=unguard(bs, Q, "s"))
    for name, buf, n, on in (("a", ba, Q, want_a), ("b", bb, Q, want_b), ("cluster_sum", bsum, K, want_cluster),
                             ("cluster_cnt", bcnt, K, want_cluster), ("skipped", bskip, 1, want_cluster)):
        got = unguard(buf, n, name)
        if on:
            out[name] = got
        else:
            assert (got == (ISENT if buf.dtype == torch.int64 else SENTINEL)).all(), "%s is NULL and was written" % name
    return out


def run(metric, q, ql, g, seg, K, P, N=None):
    """scan + finish from numpy -> (part_a, part_b, finish's dict)"""
    N = len(g) if N is None else N
    pa, pb = raw_scan(metric, f32(q), i64(ql), f32(g), i64(seg), N, K, P)
    return pa, pb, raw_finish(pa, pb, ql, seg, K, N)


_CASES = {}


def grouped_case(name):
    """the shared inputs and references of one case, computed once: g, key, seg, K, and per metric the kernel's fp32 distances, the
    float64 reference (s, a, b) and the allowances"""
    c = _CASES.get(name)
    if c is None:
        if name == "boundary":
            (x, lab), K = R.boundary_case(), R.BOUNDARY[1]
        else:
            x, lab = R.case(*name)
            K = name[1]
        g, key, order, seg = R.grouped(x, lab, K)
        c = dict(x=x, lab=lab, g=g, key=key, order=order, seg=seg, K=K, v32={}, ref={}, tol={})
        for metric in (R.EUCLID, R.SQEUCLID):
            c["v32"][metric] = R.distances(metric, g, g, fp32=True)
            c["ref"][metric] = R.dense(R.distances(metric, g, g), key, seg, K)
            c["tol"][metric] = R.allowance(metric, g, key, g, seg, K)
        _CASES[name] = c
    return c


# ================================================================================================ the scan
@pytest.mark.parametrize("name", R.SHAPES_GPU + ["boundary"], ids=str)
def test_scan_in_kernel_order_and_against_float64(name):
    """part_a / part_b bit-equal to the kernel-order restatement for P = 1, 2, 3, 7, 64 (P > K: blocks that own no cluster write
    (0, +inf)); s, a, b bit-equal across those P and to the restatement's finish; within the 8x allowance of float64; both metrics"""
    c = grouped_case(name)
    g, key, seg, K = c["g"], c["key"], c["seg"], c["K"]
    N = len(g)
    for metric in (R.EUCLID, R.SQEUCLID):
        first = None
        for P in R.P_LIST:
            pa, pb, fin = run(metric, g, key, g, seg, K, P)
            wa, wb = R.ordered_parts(metric, g, key, g, seg, K, P, V=c["v32"][metric])
            assert same(pa, wa) and same(pb, wb), (name, metric, P)
            if P > K:
                assert not pa[K:].any() and np.isposinf(pb[K:]).all()
            ws, wa_, wb_ = R.finish_rows(wa, wb, key, seg, K, N)
            assert same(fin["s"], ws) and same(fin["a"], wa_) and same(fin["b"], wb_), (name, metric, P)
            if first is None:
                first = fin
            assert all(same(fin[k], first[k]) for k in ("s", "a", "b")), (name, metric, P)
        (ts, ta, tb), errs = c["tol"][metric]
        rs, ra, rb = c["ref"][metric]
        fin_mask = np.isfinite(rs)
        assert np.array_equal(np.isnan(first["s"]), np.isnan(rs))
        es, ea, eb = (float(np.abs(first[k][fin_mask] - r[fin_mask]).max()) if fin_mask.any() else 0.0 for k, r in (("s", rs), ("a", ra), ("b", rb)))
        print("FIG sil %s metric=%d: err s %.3e a %.3e b %.3e, allowances %.3e %.3e %.3e (fp32 restatement %.3e %.3e %.3e)" % (
            (str(name), metric, es, ea, eb, ts, ta, tb) + errs))
        assert es <= ts and ea <= ta and eb <= tb
        sums, cnts, skipped = R.cluster_sums(first["s"], key, K)
        assert same(first["cluster_sum"], sums) and np.array_equal(first["cluster_cnt"], cnts) and first["skipped"][0] == skipped
        assert np.array_equal(cnts, seg[1:] - seg[:-1]) and skipped == 0          # every row of these cases has a value


def test_cuts_repeats_and_other_queries():
    c = grouped_case((130, 10, 16))
    g, key, seg, K = c["g"], c["key"], c["seg"], c["K"]
    N = len(g)
    for metric in (R.EUCLID, R.SQEUCLID):
        pa, pb, whole = run(metric, g, key, g, seg, K, 2)
        pa2, pb2, again = run(metric, g, key, g, seg, K, 2)
        assert same(pa, pa2) and same(pb, pb2) and all(same(whole[k], again[k]) for k in whole)
        # the queries cut 1 + 64 + rest: the same bits
        for lo, hi in ((0, 1), (1, 65), (65, N)):
            part = run(metric, g[lo:hi], key[lo:hi], g, seg, K, 3)[2]
            assert all(same(part[k], whole[k][lo:hi]) for k in ("s", "a", "b")), (metric, lo, hi)
        # Q != N: a shuffled subset of the gallery's rows as queries
        perm = np.random.RandomState(4510).permutation(N)
        for Q in (1, 63, 65):
            idx = perm[:Q]
            pa, pb, sub = run(metric, g[idx], key[idx], g, seg, K, 3)
            wa, wb = R.ordered_parts(metric, g[idx], key[idx], g, seg, K, 3, V=c["v32"][metric][idx])
            assert same(pa, wa) and same(pb, wb)
            assert all(same(sub[k], whole[k][idx]) for k in ("s", "a", "b")), (metric, Q)
            sums, cnts, skipped = R.cluster_sums(sub["s"], key[idx], K)
            assert same(sub["cluster_sum"], sums) and np.array_equal(sub["cluster_cnt"], cnts) and sub["skipped"][0] == skipped


@pytest.mark.parametrize("D", (1, 17))
def test_integer_data_is_exact(D):
    x, lab, t = R.integer_case(D)
    K, scale = 4, 1 if D == 1 else 2
    g, key, order, seg = R.grouped(x, lab, K)
    for metric in (R.EUCLID, R.SQEUCLID):
        want = R.integer_silhouette(t, scale, lab, K, metric)
        for P in (1, 3):
            fin = run(metric, g, key, g, seg, K, P)[2]
            for k, w in zip(("s", "a", "b"), want):
                assert np.array_equal(fin[k], w[order]), (D, metric, P, k)


# ================================================================================================ special cases
def test_special_cases():
    c = grouped_case((130, 10, 16))
    g, key, seg, K = c["g"], c["key"], c["seg"], c["K"]
    N, metric = len(g), R.EUCLID
    clean_a, clean_b, clean = run(metric, g, key, g, seg, K, 3)
    # one non-empty cluster: no value anywhere, every row is skipped
    one = np.zeros(K + 1, dtype=np.int64)
    one[1:] = N
    fin = run(metric, g, np.zeros(N, dtype=np.int64), g, one, K, 3)[2]
    assert np.isnan(fin["s"]).all() and np.isposinf(fin["b"]).all() and fin["skipped"][0] == N and not fin["cluster_cnt"].any()
    assert same(fin["a"], R.finish_rows(*R.ordered_parts(metric, g, np.zeros(N, dtype=np.int64), g, one, K, 3, V=c["v32"][metric]),
                                        np.zeros(N, dtype=np.int64), one, K, N)[1])
    # query labels out of range: NaN, b the minimum over ALL clusters, the other rows untouched
    ql = key.copy()
    ql[[3, 70]] = [-1, K]
    pa, pb, fin = run(metric, g, ql, g, seg, K, 3)
    ws, wa, wb = R.finish_rows(*R.ordered_parts(metric, g, ql, g, seg, K, 3, V=c["v32"][metric]), ql, seg, K, N)
    assert same(fin["s"], ws) and same(fin["a"], wa) and same(fin["b"], wb)
    assert np.isnan(fin["s"][[3, 70]]).all() and np.isnan(fin["a"][[3, 70]]).all() and fin["skipped"][0] == 2
    keep = np.ones(N, dtype=bool)
    keep[[3, 70]] = False
    assert same(fin["s"][keep], clean["s"][keep]) and (fin["b"][[3, 70]] <= clean["b"][[3, 70]]).all()
    # a NaN gallery row reaches exactly the sums that read it: the state that owns its cluster -- the own sum of that cluster's rows,
    # the running minimum of all others -- and no other state
    bad = int(seg[4]) + 1
    cl = 4
    assert seg[cl + 1] - seg[cl] >= 2
    gb = g.copy()
    gb[bad, 5] = np.nan
    pa, pb = raw_scan(metric, f32(g), i64(key), f32(gb), i64(seg), N, K, 3)
    owner = cl % 3
    others = [s_ for s_ in range(3) if s_ != owner]
    assert same(pa[others], clean_a[others]) and same(pb[others], clean_b[others])
    mine = key == cl
    assert np.isnan(pa[owner][mine]).all() and same(pa[owner][~mine], clean_a[owner][~mine])
    assert np.isnan(pb[owner][~mine]).all() and same(pb[owner][mine], clean_b[owner][mine])
    V32 = c["v32"][metric].copy()
    V32[:, bad] = np.nan
    wa, wb = R.ordered_parts(metric, g, key, gb, seg, K, 3, V=V32)
    assert same(pa, wa) and same(pb, wb)
    assert np.isnan(raw_finish(pa, pb, key, seg, K, N)["s"]).all()
    # seg[K] beyond N and seg[0] below 0 are clipped; the rows behind N hold huge values: reading them would show
    big = np.concatenate([g, np.full((70, g.shape[1]), 1e30)])
    last = int(np.max(np.nonzero(seg[1:] - seg[:-1])[0]))          # the last non-empty cluster
    wild = seg.copy()
    wild[last + 1:] = N + 50
    wild[0] = -5
    assert wild[last + 1] > N and seg[last + 1] == N
    pa, pb = raw_scan(metric, f32(g), i64(key), f32(big), i64(wild), N, K, 3)
    assert same(pa, clean_a) and same(pb, clean_b)
    fin = raw_finish(pa, pb, key, wild, K, N)
    assert all(same(fin[k], clean[k]) for k in clean)
    # every subset of the optional outputs: s is the same
    for want_a in (True, False):
        for want_b in (True, False):
            for want_cluster in (True, False):
                fin = raw_finish(clean_a, clean_b, key, seg, K, N, want_a, want_b, want_cluster)
                assert all(same(fin[k], clean[k]) for k in fin)


# ================================================================================================ sv_sil_finish
def test_finish_follows_the_restatement():
    rs = np.random.RandomState(4520)
    P, Q, K, N = 7, 600, 6, 1000
    seg = np.array([-3, 100, 100, 101, 400, 900, 1200], dtype=np.int64)          # an empty cluster, a singleton, both ends clipped
    ql = rs.randint(-1, K + 1, Q)
    owner = rs.randint(0, P, Q)
    pa = np.where(np.arange(P)[:, None] == owner[None, :], rs.rand(P, Q) * 50.0, 0.0)
    pb = rs.rand(P, Q) * 3.0
    pb[rs.rand(P, Q) < 0.3] = np.inf
    pb[:, 17] = np.inf                                          # no other cluster
    pb[3, 40] = np.nan
    pa[owner[41], 41] = np.nan
    pa[:, 50], pb[:, 50] = 0.0, 0.0                             # a = b = 0
    ql[[17, 40, 41, 50]] = [0, 3, 3, 4]
    fin = raw_finish(pa, pb, ql, seg, K, N)
    ws, wa, wb = R.finish_rows(pa, pb, ql, seg, K, N)
    assert same(fin["s"], ws) and same(fin["a"], wa) and same(fin["b"], wb)
    assert np.isnan(fin["s"][[17, 40, 41]]).all() and fin["s"][50] == 0.0
    assert (fin["s"][(ql == 2) & np.isfinite(wb)] == 0.0).all() and np.isnan(fin["s"][(ql == 1) | (ql < 0) | (ql >= K)]).all()
    sums, cnts, skipped = R.cluster_sums(fin["s"], ql, K)
    assert same(fin["cluster_sum"], sums) and np.array_equal(fin["cluster_cnt"], cnts) and fin["skipped"][0] == skipped > 0
    assert cnts.sum() + skipped == Q and cnts.max() > 64
    one = raw_finish(np.array([[3.0]]), np.array([[2.0]]), np.array([0]), np.array([0, 4, 8]), 2, 8)      # Q = 1
    assert one["s"][0] == (2.0 - 1.0) / 2.0 and one["a"][0] == 1.0 and one["cluster_sum"].tolist() == [0.5, 0.0]


# ================================================================================================ sv_cluster_spread
def raw_spread(x, lab, c, K, want_d2=True, want_stat=True):
    N, D = x.shape
    bd, bstat, bcnt = torch.full((N + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev()), guarded(2 * K), guarded(K, torch.int64)
    dx, dlab, dc = f32(x), i64(lab), f32(c)
    L.call("sv_cluster_spread", p(dx), p(dlab), N, D, p(dc), K, p(bd[GUARD:]) if want_d2 else None,
           p(bstat[GUARD:]) if want_stat else None, p(bcnt[GUARD:]) if want_stat else None, st())
    torch.cuda.synchronize()
    d2, stat, cnt = unguard(bd, N, "d2"), unguard(bstat, 2 * K, "stat").reshape(K, 2), unguard(bcnt, K, "cnt")
    if not want_d2:
        assert (d2 == SENTINEL).all()
    if not want_stat:
        assert (stat == SENTINEL).all() and (cnt == ISENT).all()
    return d2, stat, cnt


@pytest.mark.parametrize("N,K,D", [(5, 2, 1), (300, 7, 17), (70, 3, 128), (600, 2, 33)])
def test_cluster_spread(N, K, D):
    x = R.rows(N, D, 4530 + D)
    c = R.rows(K, D, 4531 + D)
    lab = np.random.RandomState(4532 + N).randint(0, K, N)
    lab[[0, N - 1]] = [-1, K]                                   # out of range: NaN, in no sum
    d2, stat, cnt = raw_spread(x, lab, c, K)
    wd2, wstat, wcnt = R.spread(x, lab, c, K)
    assert same(d2, wd2) and np.isnan(d2[[0, N - 1]]).all() and same(stat, wstat) and np.array_equal(cnt, wcnt)
    full = S.pairwise_distance(f32(x), None, f32(c), None, "euclid").cpu().numpy()
    ok = (lab >= 0) & (lab < K)
    assert same(d2[ok], full[np.arange(N)[ok], lab[ok]])
    assert same(raw_spread(x, lab, c, K, want_d2=False)[1], stat) and same(raw_spread(x, lab, c, K, want_stat=False)[0], d2)
    # integer data: exact
    rs = np.random.RandomState(4533 + N)
    xi, ci = rs.randint(-9, 10, (N, D)).astype(np.float64), rs.randint(-9, 10, (K, D)).astype(np.float64)
    li = rs.randint(0, K, N)
    d2, stat, cnt = raw_spread(xi, li, ci, K)
    exact = ((xi - ci[li]) ** 2).sum(axis=1)
    assert np.array_equal(d2.astype(np.float64), exact)
    assert np.array_equal(stat[:, 0], [exact[li == k].sum() for k in range(K)]) and np.array_equal(cnt, np.bincount(li, minlength=K))
    if D == 1:                                                  # (x - c)^2 is a perfect square: the roots are integers too
        assert np.array_equal(stat[:, 1], [np.abs(xi - ci[li])[li == k].sum() for k in range(K)])


# ================================================================================================ the Python layer
def counting(monkeypatch):
    reads = []
    for name in ("cpu", "item", "tolist"):
        monkeypatch.setattr(torch.Tensor, name, (lambda real: lambda self, *a, **k: (reads.append(1), real(self, *a, **k))[1])(getattr(torch.Tensor, name)))
    return reads


def test_silhouette_samples_in_the_callers_order(monkeypatch):
    x, lab = R.case(193, 65, 17)
    lab = lab.copy()
    lab[[5, 100]] = [-1, 65]                                    # in no cluster
    x = x.copy()
    x[77, 3] = np.inf                                           # not finite: in no cluster
    K = 65
    reads = counting(monkeypatch)
    got = V.silhouette_samples(f32(x), i64(lab), K)
    sub, idx = V.silhouette_samples(f32(x), i64(lab), K, queries=50, seed=3)
    everyone, idx_all = V.silhouette_samples(f32(x), i64(lab), K, queries=193, seed=3)
    monkeypatch.undo()
    assert not reads, "silhouette_samples read from the device"
    assert got.dtype == torch.float64 and tuple(got.shape) == (193,) and got.is_cuda
    got = got.cpu().numpy()
    g, key, order, seg = R.grouped(x, lab, K)
    assert seg[K] == 190
    P = V.default_partials(193, 193, K)
    with np.errstate(invalid="ignore"):
        V32 = R.distances(R.EUCLID, g, g, fp32=True)
    ws = R.finish_rows(*R.ordered_parts(R.EUCLID, g, key, g, seg, K, P, V=V32), key, seg, K, 193)[0]
    want = np.empty(193)
    want[order] = ws
    assert same(got, want) and np.isnan(got[[5, 77, 100]]).all() and np.isfinite(np.delete(got, [5, 77, 100])).all()
    keep = np.ones(193, dtype=bool)
    keep[[5, 77, 100]] = False
    ref = R.silhouette_samples(x[keep], lab[keep], K)           # float64, without those rows altogether
    gk, kk, _, sk = R.grouped(x[keep], lab[keep], K)
    tol = R.allowance(R.EUCLID, gk, kk, gk, sk, K)[0][0]
    err = float(np.abs(got[keep] - ref).max())
    print("FIG silhouette_samples 193 x 17, K = 65: err %.3e allowance %.3e" % (err, tol))
    assert err <= tol
    assert np.array_equal(idx.cpu().numpy(), V.query_indices(193, 50, 3).numpy()) and same(sub.cpu().numpy(), got[idx.cpu().numpy()])
    assert same(everyone.cpu().numpy(), got[idx_all.cpu().numpy()]) and sorted(idx_all.cpu().tolist()) == list(range(193))
    sq = V.silhouette_samples(f32(x), i64(lab), K, metric="sqeuclid").cpu().numpy()
    assert not same(sq, got) and np.array_equal(np.isnan(sq), np.isnan(got))


def test_silhouette_grouped_equals_the_calls_by_hand_and_a_replayed_graph():
    c = grouped_case((130, 10, 16))
    g, key, seg, K = c["g"], c["key"], c["seg"], c["K"]
    N = len(g)
    s, csum, ccnt, skipped = V.silhouette_grouped(f32(g), i64(key), f32(g), i64(seg), K)
    assert s.dtype == csum.dtype == torch.float64 and ccnt.dtype == skipped.dtype == torch.int64
    fin = run(R.EUCLID, g, key, g, seg, K, V.default_partials(N, N, K))[2]
    assert same(s.cpu().numpy(), fin["s"]) and same(csum.cpu().numpy(), fin["cluster_sum"])
    assert np.array_equal(ccnt.cpu().numpy(), fin["cluster_cnt"]) and int(skipped) == fin["skipped"][0]
    for P in (1, 64):
        assert torch.equal(V.silhouette_grouped(f32(g), i64(key), f32(g), i64(seg), K, P=P)[0], s)
    # under graph capture, replayed on new rows and a new seg of the same shapes
    x2, lab2 = R.case(130, 10, 16, seed=11)
    g2, key2, _, seg2 = R.grouped(x2, lab2, K)
    assert not np.array_equal(seg2, seg)
    sets = [(f32(g), i64(key), i64(seg)), (f32(g2), i64(key2), i64(seg2))]
    sg, sk, ss = (t.clone() for t in sets[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                               # warm-up outside the capture
        V.silhouette_grouped(sg, sk, sg, ss, K)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = V.silhouette_grouped(sg, sk, sg, ss, K)
    for rows_, key_, seg_ in (sets[1], sets[0]):
        sg.copy_(rows_)
        sk.copy_(key_)
        ss.copy_(seg_)
        graph.replay()
        torch.cuda.synchronize()
        eager = V.silhouette_grouped(rows_, key_, rows_, seg_, K)
        assert all(torch.equal(a, b) for a, b in zip(out, eager))
    assert not torch.equal(V.silhouette_grouped(*[sets[0][i] for i in (0, 1, 0, 2)], K)[0], V.silhouette_grouped(*[sets[1][i] for i in (0, 1, 0, 2)], K)[0])


def test_score_and_indices_read_the_host_once(monkeypatch):
    x, lab = R.case(257, 10, 128)
    K = 10
    reads = counting(monkeypatch)
    score = V.silhouette_score(f32(x), i64(lab), K)
    n_score = len(reads)
    res = V.validity_indices(f32(x), i64(lab), K)
    n_res = len(reads) - n_score
    cent, cnt, within, mean_dist = V.cluster_spread(f32(x), i64(lab), K)
    n_spread = len(reads) - n_score - n_res
    monkeypatch.undo()
    assert n_score == 1 and n_res == 1 and n_spread == 0, (n_score, n_res, n_spread)
    g, key, order, seg = R.grouped(x, lab, K)
    ref = R.silhouette_samples(x, lab, K)
    tol = R.allowance(R.EUCLID, g, key, g, seg, K)[0][0]
    sizes = np.bincount(lab, minlength=K)
    print("FIG silhouette_score 257 x 128, K = 10: %.9e (float64 %.9e, allowance %.2e)" % (score["score"], ref.mean(), tol))
    assert abs(score["score"] - ref.mean()) <= tol and score["skipped"] == 0 and np.array_equal(score["counts"], sizes)
    for k in range(K):
        if sizes[k]:
            assert abs(score["per_cluster"][k] - ref[lab == k].mean()) <= tol
        else:
            assert np.isnan(score["per_cluster"][k])
    assert res["silhouette"] == score["score"] and res["clusters"] == int((sizes > 0).sum()) and res["n"] == 257
    (tch, tdb), (ch, db) = R.indices_allowance(x, lab, K)
    print("FIG validity_indices 257 x 128, K = 10: calinski_harabasz %.9e (float64 %.9e, allowance %.2e) davies_bouldin %.9e (%.9e, %.2e)" % (
        res["calinski_harabasz"], ch, tch, res["davies_bouldin"], db, tdb))
    assert abs(res["calinski_harabasz"] - ch) <= tch and abs(res["davies_bouldin"] - db) <= tdb
    # cluster_spread: the centroids are sv_kmeans_finish's, the spread sv_cluster_spread's about them
    c64, n64 = R.centroids_of(x, lab, K)
    assert np.array_equal(cnt.cpu().numpy(), n64) and np.abs(cent.double().cpu().numpy() - c64).max() <= 4 * np.spacing(np.float32(np.abs(c64).max()))
    _, wstat, wcnt = R.spread(x, lab, cent.double().cpu().numpy(), K)
    assert same(within.cpu().numpy(), wstat[:, 0]) and same(mean_dist.cpu().numpy(), np.where(wcnt > 0, wstat[:, 1] / np.maximum(wcnt, 1), 0.0))
    # a subset of the queries: an estimate from exact values
    part = V.silhouette_score(f32(x), i64(lab), K, queries=100, seed=2)
    idx = V.query_indices(257, 100, 2).numpy()
    assert abs(part["score"] - ref[idx].mean()) <= tol and np.array_equal(part["counts"], sizes)
    with pytest.raises(ValueError, match="2 non-empty clusters"):
        V.silhouette_score(f32(x), i64(np.zeros(257)), K)


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


def same_result(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(same_result(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return len(a) == len(b) and all(same_result(u, v) for u, v in zip(a, b))
    if isinstance(a, np.ndarray):
        return same(a, b)
    if isinstance(a, float):
        return a == b or (a != a and b != b)
    return a == b


@pytest.mark.parametrize("kind", KR.EVAL_KINDS)
def test_evaluate_validity_on_the_closed_form_models(kind, monkeypatch):
    model = eval_model(kind)
    xa, ya = (t.to(dev()) for t in KR.eval_images(kind)[:2])
    batches = lambda b: [(xa[i:i + b], ya[i:i + b]) for i in range(0, xa.shape[0], b)]          # noqa: E731
    K = KR.EVAL_CLASSES
    # ---- the true classes as the partition, in both spaces of the posterior
    for space in ("mu", "w2"):
        reads = counting(monkeypatch)
        res = S.evaluate_validity(model, batches(16), method="labels", space=space, chunk_rows=16)
        n_reads = len(reads)
        monkeypatch.undo()
        assert n_reads == 1, "evaluate_validity reads the host once (%d)" % n_reads
        assert same_result(res, S.evaluate_validity(model, batches(48), method="labels", space=space, chunk_rows=16))
        mu, ls = (torch.cat(t) for t in zip(*[S.encode_posterior(model, img) for img, _ in batches(16)]))
        rows_ = mu if space == "mu" else torch.cat([mu, ls.exp()], dim=1)
        x, lab = rows_.double().cpu().numpy(), ya.cpu().numpy()
        g, key, order, seg = R.grouped(x, lab, K)
        ref, tol = R.silhouette_samples(x, lab, K), R.allowance(R.EUCLID, g, key, g, seg, K)[0][0]
        (tch, tdb), (ch, db) = R.indices_allowance(x, lab, K)
        print("FIG evaluate_validity %s labels %s: silhouette %.6e (float64 %.6e, allowance %.1e) ch %.6e (%.6e, %.1e) db %.6e (%.6e, %.1e)" % (
            kind, space, res["silhouette"], ref.mean(), tol, res["calinski_harabasz"], ch, tch, res["davies_bouldin"], db, tdb))
        assert abs(res["silhouette"] - ref.mean()) <= tol and res["k"] == K and res["n"] == KR.EVAL_GALLERY and res["skipped"] == 0
        assert abs(res["calinski_harabasz"] - ch) <= tch and abs(res["davies_bouldin"] - db) <= tdb
    if kind != "svhn":
        feat = S.evaluate_validity(model, batches(16), method="labels", space="features", chunk_rows=16)
        assert feat["space"] == "features" and feat["n"] == KR.EVAL_GALLERY and -1.0 <= feat["silhouette"] <= 1.0
    else:
        with pytest.raises(ValueError, match="features"):
            S.evaluate_validity(model, batches(16), method="labels", space="features")
    # ---- the model's own discrete code
    with torch.no_grad():
        own = torch.cat([model.encode(img)[2].argmax(dim=1) for img, _ in batches(16)])
    mu = torch.cat([S.encode_posterior(model, img)[0] for img, _ in batches(16)])          # the evaluator's chunks: the same bits
    if int((torch.bincount(own, minlength=K) > 0).sum()) >= 2:
        res = S.evaluate_validity(model, batches(16), method="posterior", chunk_rows=16)
        assert same_result(res, S.evaluate_validity(model, batches(32), method="posterior", chunk_rows=16))
        assert same_result({k: v for k, v in res.items() if k not in ("method", "space", "k")}, V.validity_indices(mu, own, K))
    else:                                                       # an untrained code may name one class only: no index exists
        with pytest.raises(ValueError, match="non-empty clusters"):
            S.evaluate_validity(model, batches(16), method="posterior", chunk_rows=16)
    # ---- k-means, one k and the sweep
    one = S.evaluate_validity(model, batches(16), method="kmeans", k=3, chunk_rows=16, seed=1, max_iter=5, tol=None)
    cluster = S.KMeans(3, mu.shape[1], seed=1).fit(mu, max_iter=5, tol=None).predict(mu)
    assert same_result({k: v for k, v in one.items() if k not in ("method", "space", "k")}, V.validity_indices(mu, cluster, 3, seed=1))
    sweep = S.evaluate_validity(model, batches(16), method="kmeans", k=[2, 3, 4], chunk_rows=16, seed=1, max_iter=5, tol=None)
    assert same_result(sweep, S.evaluate_validity(model, batches(48), method="kmeans", k=[2, 3, 4], chunk_rows=16, seed=1, max_iter=5, tol=None))
    assert sweep["ks"] == [2, 3, 4] and same_result(sweep["results"][1], one)
    scores = [r["silhouette"] for r in sweep["results"]]
    assert sweep["best_k"] == sweep["ks"][int(np.argmax(scores))]
    with pytest.raises(NotImplementedError):
        S.evaluate_validity(model.train(), batches(16))
    model.eval()
