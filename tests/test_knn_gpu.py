"""Posterior distances and k-NN search on a real MI355X: sv_pairdist, sv_knn_scan and sv_knn_vote through the C ABI against the float64
restatement of tests/_knn_ref.py (pinned to the reference's own outputs by tests/test_knn_cpu.py), then the Python layer
(shot_vae_amd.neighbors, evaluate_knn).

Allowances follow the project's 8x rule and are measured when the test runs, never taken from a GPU result: 8 x the error of the fp32
numpy restatement against float64 on posterior() rows of the case's dimension (R.tolerance_for), or on the case's own inputs where
they are many (the fixture's large case, the models' encode outputs).  Inputs: mu ~ N(0, 1), log sigma ~ U(-1, 0.5) (closed forms).
Outputs are pre-filled (NaN / -7) and carry guard rows.

evaluate_knn runs under "euclid" and "w2", not "kl": see tests/_knn_ref.py (EVAL_CASES) for the measured reason.

Measured on an MI355X, error (allowance): sv_pairdist against the fixture's large case kl 4.0e-5 (5.8e-4), w2 4.2e-5 (4.4e-4), euclid
3.9e-5 (3.6e-4), cosine 2.3e-10 (5.6e-9), its small case 3.2e-6 .. 5.9e-6 (4.3e-5 .. 1.1e-4), cosine 1.1e-8 (7.1e-7); |KL(x || x)|
9.5e-7 (5.8e-4), Euclid / W2 exactly 0; sv_knn_scan slot values at D = 128 / 130 3.0e-5 .. 5.0e-5 (3.9e-4 .. 5.8e-4), at D = 1 / 7
8.9e-10 .. 2.2e-6 (2.1e-5 .. 1.4e-4); weighted votes 2.8e-8 .. 3.5e-7 (5.4e-7 .. 3.8e-6); evaluate_knn 0 of 48 rows undecided in the three
cases."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import shot_vae_amd as S                                        # noqa: E402
from shot_vae_amd import _lib as L                              # noqa: E402
from shot_vae_amd import neighbors as NB                        # noqa: E402
from tests import _cases as T                                   # noqa: E402
from tests import _knn_ref as R                                 # noqa: E402
from tests.golden import make_dist_goldens as G                 # noqa: E402

GUARD = 3
PAIR_SHAPES = [(1, 1, 1, 0), (3, 5, 7, 0), (33, 65, 128, 0), (65, 257, 130, 0), (3, 5, 7, 9), (33, 65, 128, 80)]     # Q, N, D, ldo (0: N)


def dev():
    return torch.device("cuda:0")


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def f32(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev())


def rows(n, D, stream):
    """posterior() rows as (float64 numpy mu, ls)"""
    return R.posterior(n, D, stream)


def pairdist(metric, mu1, ls1, mu2, ls2, ldo=0):
    """sv_pairdist into a NaN-filled [Q + GUARD][ldo] buffer -> float64 numpy [Q, N]; the pad columns and guard rows stay NaN"""
    Q, D = mu1.shape
    N = mu2.shape[0]
    ldo = ldo or N
    needs = metric in ("kl", "w2")
    out = torch.full((Q + GUARD, ldo), float("nan"), dtype=torch.float32, device=dev())
    qm, ql = f32(mu1), f32(ls1) if needs else None          # (held in names: a temporary's memory is reused by the next one)
    gm, gl = f32(mu2), f32(ls2) if needs else None
    L.call("sv_pairdist", R.CODE[metric], p(qm), p(ql), Q, p(gm), p(gl), N, D, p(out), ldo, st())
    torch.cuda.synchronize()
    assert torch.isnan(out[Q:]).all() and torch.isnan(out[:Q, N:]).all(), "sv_pairdist wrote outside its matrix"
    return out[:Q, :N].double().cpu().numpy()


def scan(metric, mu1, ls1, mu2, ls2, k, cuts=None, self0=-1, col0=0):
    """sv_knn_scan over the gallery cut at `cuts` (row offsets; the first call has init = 1 and finds garbage in the lists) ->
    (val, idx) device tensors [Q, k]; the guard rows behind the lists stay as they were"""
    Q, D = mu1.shape
    N = mu2.shape[0]
    needs = metric in ("kl", "w2")
    qm, ql = f32(mu1), f32(ls1) if needs else None
    gm, gl = f32(mu2), f32(ls2) if needs else None
    val = torch.full((Q + GUARD, k), -7.0, dtype=torch.float32, device=dev())
    idx = torch.full((Q + GUARD, k), -7, dtype=torch.int64, device=dev())
    edges = [0] + list(cuts or []) + [N]
    for n, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        L.call("sv_knn_scan", R.CODE[metric], p(qm), p(ql), Q, p(gm[a:]), p(gl[a:]) if needs else None, b - a, D, col0 + a, self0, k, p(val),
               p(idx), 1 if n == 0 else 0, st())
    torch.cuda.synchronize()
    assert bool((val[Q:] == -7).all()) and bool((idx[Q:] == -7).all()), "sv_knn_scan wrote behind its lists"
    return val[:Q], idx[:Q]


def check_lists(metric, val, idx, ref, k, tol, col0=0, self0=-1):
    """the list properties of the issue against the float64 matrix `ref` [Q, N]"""
    val, idx = val.double().cpu().numpy(), idx.cpu().numpy()
    rval, ridx = R.topk(ref, k, metric, col0=col0, self0=self0)
    empty = -np.inf if metric == "cosine" else np.inf
    assert np.array_equal(idx >= 0, ridx >= 0), "the number of filled slots differs"
    filled = ridx >= 0
    assert (idx[~filled] == -1).all() and (val[~filled] == empty).all()
    assert np.abs(val[filled] - rval[filled]).max(initial=0.0) <= tol, "a slot's value is not the float64 k-th closest"
    rows_, _ = np.nonzero(filled)
    at = ref[rows_, idx[filled] - col0]
    assert np.abs(at - val[filled]).max(initial=0.0) <= tol, "the float64 distance at a returned index is not the returned value"
    for i in range(idx.shape[0]):
        got = idx[i][idx[i] >= 0]
        assert len(set(got.tolist())) == len(got), "an index repeats in row %d" % i
        assert self0 < 0 or self0 + i not in got
        v = val[i][idx[i] >= 0]
        assert (np.diff(v) <= 0).all() if metric == "cosine" else (np.diff(v) >= 0).all(), "row %d is not sorted" % i
    return float(np.abs(val[filled] - rval[filled]).max(initial=0.0))


# ================================================================================================ sv_pairdist
@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("Q,N,D,ldo", PAIR_SHAPES)
def test_pairdist_matches_float64(metric, Q, N, D, ldo):
    mu1, ls1 = rows(Q, D, 9901)
    mu2, ls2 = rows(N, D, 9903)
    ref = R.distances(metric, mu1, ls1, mu2, ls2)
    got = pairdist(metric, mu1, ls1, mu2, ls2, ldo)
    tol = R.tolerance_for(metric, D)
    err = float(np.abs(got - ref).max())
    print("FIG pairdist %s %s err %.3e tol %.3e max %.3e" % (metric, (Q, N, D, ldo), err, tol, np.abs(ref).max()))
    assert err <= tol


@pytest.mark.parametrize("metric,name", [("kl", "kl"), ("w2", "w2"), ("euclid", "euclid"), ("cosine", "mcosine")])
@pytest.mark.parametrize("size", sorted(G.SIZES))
def test_pairdist_matches_the_reference_fixture(metric, name, size):
    g = T.load(G.TAG)
    u1, l1, u2, l2 = G.dist_inputs(size, "f64")
    got = pairdist(metric, u1, l1, u2, l2)
    tol = R.tolerance_for(metric, G.SIZES[size][2])
    err = float(np.abs(got - g["%s_%s_f64" % (name, size)]).max())
    print("FIG fixture %s %s err %.3e tol %.3e" % (metric, size, err, tol))
    assert err <= tol
    # the reference's own fp32 run is as far from float64 as the rule allows this kernel to be
    assert float(np.abs(g["%s_%s_f32" % (name, size)].astype(np.float64) - g["%s_%s_f64" % (name, size)]).max()) <= tol


def test_pairdist_self_distance():
    mu, ls = rows(65, 128, 9905)
    for metric in ("euclid", "w2"):
        assert (np.diag(pairdist(metric, mu, ls, mu, ls)) == 0.0).all(), metric
    d = np.abs(np.diag(pairdist("kl", mu, ls, mu, ls))).max()
    print("FIG self kl %.3e tol %.3e" % (d, R.tolerance_for("kl", 128)))
    assert d <= R.tolerance_for("kl", 128)


# ================================================================================================ sv_knn_scan
SCAN_CASES = [("kl", 1, 1, 1, 1), ("kl", 33, 257, 5, 7), ("w2", 65, 1000, 20, 128), ("euclid", 33, 5, 5, 130), ("cosine", 65, 257, 256, 7),
              ("kl", 33, 5, 20, 128), ("kl", 65, 1000, 256, 130), ("cosine", 1, 1000, 1, 128), ("w2", 1, 257, 256, 1),
              ("euclid", 65, 1, 1, 7), ("w2", 33, 257, 256, 128), ("euclid", 65, 1000, 5, 1), ("cosine", 33, 5, 20, 130)]


@pytest.mark.parametrize("metric,Q,N,k,D", SCAN_CASES)
def test_knn_scan_values(metric, Q, N, k, D):
    mu1, ls1 = rows(Q, D, 9907)
    mu2, ls2 = rows(N, D, 9909)
    ref = R.distances(metric, mu1, ls1, mu2, ls2)
    val, idx = scan(metric, mu1, ls1, mu2, ls2, k)
    tol = R.tolerance_for(metric, D)
    err = check_lists(metric, val, idx, ref, k, tol)
    print("FIG scan %s %s err %.3e tol %.3e" % (metric, (Q, N, k, D), err, tol))
    # the scan and the matrix kernel give the same bits for the same pair
    got = torch.from_numpy(pairdist(metric, mu1, ls1, mu2, ls2)).float()
    i = idx.cpu().clamp(min=0)
    assert torch.equal(torch.gather(got, 1, i)[idx.cpu() >= 0], val.cpu()[idx.cpu() >= 0])


@pytest.mark.parametrize("Q,N,k,D", [(33, 257, 20, 7), (65, 1000, 256, 7), (1, 1000, 5, 1), (33, 257, 256, 130), (65, 5, 20, 7)])
def test_knn_scan_exact_ties(Q, N, k, D):
    """small-integer means under Euclid: fp32 is exact, ties are many -- indices EQUAL to the restatement's, tie order included"""
    from oracle import closed_form as CF
    mu1 = np.floor(CF.uniform((Q, D), 9911, -2.0, 3.0).numpy().astype(np.float64))
    mu2 = np.floor(CF.uniform((N, D), 9912, -2.0, 3.0).numpy().astype(np.float64))
    ref = R.distances("euclid", mu1, None, mu2, None)
    rval, ridx = R.topk(ref, k, "euclid")
    assert max((np.diff(np.sort(r)) == 0).sum() for r in ref) >= min(N, 8) // 2, "the case has no ties"
    for cuts in (None, [1, 3] if N > 3 else None, [N // 2]):
        val, idx = scan("euclid", mu1, None, mu2, None, k, cuts=cuts)
        assert np.array_equal(idx.cpu().numpy(), ridx) and np.array_equal(val.double().cpu().numpy(), rval)


@pytest.mark.parametrize("metric,k", [("kl", 20), ("kl", 256), ("w2", 5), ("euclid", 1), ("cosine", 20), ("cosine", 200)])
def test_knn_scan_chunking_is_bit_identical(metric, k):
    Q, N, D = 65, 1000, 128
    mu1, ls1 = rows(Q, D, 9913)
    mu2, ls2 = rows(N, D, 9915)
    one = scan(metric, mu1, ls1, mu2, ls2, k)
    for cuts in ([1, 257], list(range(100, 1000, 100))):
        got = scan(metric, mu1, ls1, mu2, ls2, k, cuts=cuts)
        assert torch.equal(one[0], got[0]) and torch.equal(one[1], got[1]), (metric, k, cuts)
    check_lists(metric, one[0], one[1], R.distances(metric, mu1, ls1, mu2, ls2), k, R.tolerance_for(metric, D))


@pytest.mark.parametrize("metric", R.METRICS)
def test_knn_scan_leave_one_out(metric):
    """the queries are gallery rows 300 .. 332: scanned as a second chunk (col0 = 300) with self0 = 300, nobody finds itself"""
    Q, D, k, off = 33, 128, 5, 300
    mu2, ls2 = rows(off + Q, D, 9917)
    mu1, ls1 = mu2[off:], ls2[off:]
    ref = R.distances(metric, mu1, ls1, mu2, ls2)
    val, idx = scan(metric, mu1, ls1, mu2, ls2, k, cuts=[off], self0=off)
    check_lists(metric, val, idx, ref, k, R.tolerance_for(metric, D), self0=off)
    # without the exclusion every query's nearest row is itself (cosine: the reference's formula has no such property)
    if metric != "cosine":
        val, idx = scan(metric, mu1, ls1, mu2, ls2, k, cuts=[off])
        assert np.array_equal(idx[:, 0].cpu().numpy(), off + np.arange(Q))
    # a chunk of its own, addressed by col0: the same lists as the cut scan
    val2, idx2 = scan(metric, mu1, ls1, mu2[off:], ls2[off:], k, col0=off, self0=off)
    check_lists(metric, val2, idx2, ref[:, off:], k, R.tolerance_for(metric, D), col0=off, self0=off)


@pytest.mark.parametrize("metric", R.METRICS)
def test_knn_scan_never_returns_nan_or_infinite_rows(metric):
    Q, N, D = 5, 70, 7
    mu1, ls1 = rows(Q, D, 9919)
    mu2, ls2 = rows(N, D, 9921)
    mu2[3] = np.nan                                        # a gallery row of NaN
    bad = [3]
    if metric in ("kl", "w2"):
        ls2[66] = np.inf                                   # sigma = +inf: KL and W2 are +inf
        bad.append(66)
    mu1[2] = np.nan                                        # a NaN query
    val, idx = scan(metric, mu1, ls1, mu2, ls2, N, cuts=[64])
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    empty = -np.inf if metric == "cosine" else np.inf
    assert (idx[2] == -1).all() and (val[2] == empty).all()
    for i in (0, 1, 3, 4):
        assert sorted(idx[i][idx[i] >= 0].tolist()) == [j for j in range(N) if j not in bad]
        assert (idx[i][N - len(bad):] == -1).all() and (val[i][N - len(bad):] == empty).all() and np.isfinite(val[i][:N - len(bad)]).all()


def test_knn_scan_agrees_with_sv_optimal_match():
    """metric KL, k = 2, gallery = queries, B = 64: column 1 of best_idx is sv_optimal_match's pairing on every row whose 2nd and 3rd
    smallest float64 KL are more than 4 tolerances apart; at most 10 % of the rows may be closer than that"""
    B, D = 64, 128
    mu, ls = rows(B, D, 9923)
    ref = R.distances("kl", mu, ls, mu, ls)
    tol = R.tolerance_for("kl", D)
    srt = np.sort(ref, axis=1)
    decided = (srt[:, 2] - srt[:, 1]) > 4.0 * tol
    assert int((~decided).sum()) <= B // 10
    val, idx = scan("kl", mu, ls, mu, ls, 2)
    match = torch.full((B,), -7, dtype=torch.int64, device=dev())
    dmu, dls = f32(mu), f32(ls)
    L.call("sv_optimal_match", p(dmu), p(dls), B, D, p(match), st())
    torch.cuda.synchronize()
    assert np.array_equal(idx[:, 1].cpu().numpy()[decided], match.cpu().numpy()[decided])
    assert np.array_equal(idx[:, 0].cpu().numpy(), np.arange(B))          # KL(x || x) = 0 is every row's minimum


# ================================================================================================ sv_knn_vote
def vote(val, idx, g_label, K, mode, tau=1.0, q_label=None, counts=None, confusion=None, want_votes=True):
    Q, k = idx.shape
    pred = torch.full((Q + GUARD,), -7, dtype=torch.int64, device=dev())
    votes = torch.full((Q + GUARD, K), float("nan"), dtype=torch.float32, device=dev()) if want_votes else None
    L.call("sv_knn_vote", p(val), p(idx), Q, k, p(g_label), g_label.numel(), K, mode, float(tau), p(q_label), p(pred), p(votes), p(counts),
           p(confusion), st())
    torch.cuda.synchronize()
    assert bool((pred[Q:] == -7).all()) and (votes is None or torch.isnan(votes[Q:]).all())
    return pred[:Q].cpu().numpy(), (votes[:Q].double().cpu().numpy() if want_votes else None)


def vote_case(metric, Q, N, k, K, D=7):
    """lists of a real scan (with empty tails when k > N), gallery labels with values outside [0, K), two rows without any voter"""
    mu1, ls1 = rows(Q, D, 9925)
    mu2, ls2 = rows(N, D, 9927)
    val, idx = R.topk(R.distances(metric, mu1, ls1, mu2, ls2), k, metric)
    val = val.astype(np.float32).astype(np.float64)
    g_label = (np.arange(N) * 7 + 3) % (K + 2) - 1         # -1 .. K: both ends are outside [0, K)
    for i in {i for i in (1, Q - 1) if 0 < i < Q}:          # rows whose neighbours are all unlabelled / empty
        idx[i, :] = -1
        val[i, :] = -np.inf if metric == "cosine" else np.inf
    idx[0, 0] = N + 5                                       # an index outside the gallery casts no vote
    return val, idx, g_label


@pytest.mark.parametrize("metric,Q,N,k,K", [("euclid", 37, 300, 20, 10), ("kl", 5, 9, 20, 3), ("cosine", 9, 300, 256, 100), ("w2", 1, 70, 1, 1)])
def test_knn_vote_matches_the_restatement(metric, Q, N, k, K):
    val, idx, g_label = vote_case(metric, Q, N, k, K)
    dval, didx = f32(val), torch.from_numpy(idx).to(dev())
    dlab = torch.from_numpy(g_label).to(dev())
    rvotes, rpred = R.vote(val, idx, g_label, K, 0)
    pred, votes = vote(None, didx, dlab, K, 0)             # best_val may be NULL in mode 0
    assert np.array_equal(votes, rvotes) and np.array_equal(pred, rpred)
    assert (pred[[1, Q - 1]] == -1).all() if Q > 2 else True
    assert np.array_equal(vote(dval, didx, dlab, K, 0, want_votes=False)[0], rpred)
    # weighted: tau on the scale of the values, so that the weights neither vanish nor coincide
    fin = val[np.isfinite(val)]
    mode, tau = (2, float(np.abs(fin).max())) if metric == "cosine" else (1, float(np.median(fin)))
    rvotes, rpred = R.vote(val, idx, g_label, K, mode, tau)
    tol = 8.0 * float(np.abs(R.vote32(val, idx, g_label, K, mode, tau).astype(np.float64) - rvotes).max())
    pred, votes = vote(dval, didx, dlab, K, mode, tau)
    err = float(np.abs(votes - rvotes).max())
    print("FIG vote %s mode %d err %.3e tol %.3e max %.3e" % (metric, mode, err, tol, rvotes.max()))
    assert err <= tol
    voted = (rvotes > 0).any(axis=1)
    assert np.array_equal(pred[voted], votes[voted].argmax(axis=1)) and (pred[~voted] == -1).all()      # the first maximum of its own votes
    top2 = np.sort(rvotes, axis=1)[:, -2:] if K > 1 else np.stack([np.full(Q, -np.inf), rvotes[:, 0]], 1)
    clear = voted & ((top2[:, 1] - top2[:, 0]) > 2.0 * tol)
    assert np.array_equal(pred[clear], rpred[clear])


def test_knn_vote_counters_accumulate_exactly():
    Q, N, k, K = 37, 300, 20, 10
    val, idx, g_label = vote_case("euclid", Q, N, k, K)
    didx, dlab = torch.from_numpy(idx).to(dev()), torch.from_numpy(g_label).to(dev())
    rpred = R.vote(val, idx, g_label, K, 0)[1]
    counts = torch.zeros(2, dtype=torch.int64, device=dev())
    conf = torch.zeros(K, K, dtype=torch.int64, device=dev())
    want_counts, want_conf = np.zeros(2, dtype=np.int64), np.zeros((K, K), dtype=np.int64)
    for call in range(2):
        q_label = (np.arange(Q) * 3 + call) % (K + 3) - 1  # -1, K and K + 1 are outside [0, K): a row, never a hit, never a cell
        q_label[::2] = np.where(rpred[::2] >= 0, rpred[::2], q_label[::2])      # every other row is a hit where a prediction exists
        pred, _ = vote(None, didx, dlab, K, 0, q_label=torch.from_numpy(q_label).to(dev()), counts=counts, confusion=conf, want_votes=False)
        assert np.array_equal(pred, rpred)
        c, m = R.counters(rpred, q_label, K)
        want_counts += c
        want_conf += m
    assert np.array_equal(counts.cpu().numpy(), want_counts) and np.array_equal(conf.cpu().numpy(), want_conf)
    assert want_counts[1] == 2 * Q and 0 < want_counts[0] < 2 * Q and want_conf.sum() < 2 * Q


# ================================================================================================ the Python layer
def test_reference_drop_ins_match_the_fixture():
    g = T.load(G.TAG)
    for size in sorted(G.SIZES):
        u1, l1, u2, l2 = (f32(a) for a in G.dist_inputs(size, "f64"))
        d = G.SIZES[size][2]
        got = {"kl": NB.pairwise_norm_kl_dist_gpu(u1, l1, u2, l2), "w2": NB.pairwise_norm_wasserstein_dist_gpu(u1, l1, u2, l2),
               "euclid": NB.pairwise_square_euclidean_gpu(u1, u2),
               "meuclid": NB.calculate_mean_dist_pairwise(u1, u2, GPU_flag=True, distance="euclidean"),
               "mcosine": NB.calculate_mean_dist_pairwise(u1.cpu().numpy(), u2.cpu().numpy(), GPU_flag=True, distance="cosine")}
        for name, t in got.items():
            metric = {"meuclid": "euclid", "mcosine": "cosine"}.get(name, name)
            ref = g["%s_%s_f64" % (name, size)]
            assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == ref.shape
            assert float(np.abs(t.double().cpu().numpy() - ref).max()) <= R.tolerance_for(metric, d), (name, size)
        assert torch.equal(got["kl"], S.pairwise_distance(u1, l1, u2, l2, metric="kl"))
    with pytest.raises(NotImplementedError, match="distance manhattan not implemented"):
        NB.calculate_mean_dist_pairwise(u1, u2, GPU_flag=True, distance="manhattan")


@pytest.mark.parametrize("metric", ["kl", "cosine"])
def test_latent_index_add_in_pieces_is_bit_equal(metric):
    N, Q, D, K, k = 1500, 33, 7, 10, 20                     # 1500 rows: the buffers grow once on the way (1024 -> 2048)
    mu2, ls2 = (f32(a) for a in rows(N, D, 9929))
    mu1, ls1 = (f32(a) for a in rows(Q, D, 9931))
    lab = (torch.arange(N, device=dev()) * 7 + 3) % K
    one = S.LatentIndex(D, metric=metric, num_classes=K)
    assert one.add(mu2, ls2, lab) == 0 and len(one) == N
    three = S.LatentIndex(D, metric=metric, num_classes=K)
    firsts = [three.add(mu2[a:b], ls2[a:b], lab[a:b]) for a, b in ((0, 700), (700, 1200), (1200, N))]
    assert firsts == [0, 700, 1200] and len(three) == N
    a, b = one.search(mu1, ls1, k), three.search(mu1, ls1, k)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(one.classify(mu1, ls1, k, weights="distance", tau=5.0), three.classify(mu1, ls1, k, weights="distance", tau=5.0))
    ref = R.distances(metric, *(t.double().cpu().numpy() for t in (mu1, ls1, mu2, ls2)))
    check_lists(metric, a[0], a[1], ref, k, R.tolerance_for(metric, D))
    # leave-one-out through the index: the gallery's own rows 700 .. 732 as queries
    v, i = one.search(mu2[700:733], ls2[700:733], 3, exclude_self_from=700)
    assert not bool((i == torch.arange(700, 733, device=dev())[:, None]).any())


def test_latent_index_search_and_classify_under_graph_capture():
    N, Q, D, K, k = 300, 33, 128, 10, 20
    mu2, ls2 = (f32(a) for a in rows(N, D, 9933))
    index = S.LatentIndex(D, metric="kl", num_classes=K)
    index.add(mu2, ls2, (torch.arange(N, device=dev()) * 7 + 3) % K)
    qs = [tuple(f32(a) for a in rows(Q, D, s)) for s in (9935, 9937)]
    label = (torch.arange(Q, device=dev()) * 3) % K
    smu, sls = qs[0][0].clone(), qs[0][1].clone()
    counts = torch.zeros(2, dtype=torch.int64, device=dev())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                           # warm-up outside the capture
        index.search(smu, sls, k)
        index.classify(smu, sls, k, label=label, counts=counts)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    counts.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        val, idx = index.search(smu, sls, k)
        pred = index.classify(smu, sls, k, label=label, counts=counts)
    hits = 0
    for mu1, ls1 in (qs[1], qs[0]):                         # replayed on new queries
        smu.copy_(mu1)
        sls.copy_(ls1)
        graph.replay()
        torch.cuda.synchronize()
        ev, ei = index.search(mu1, ls1, k)
        ep = index.classify(mu1, ls1, k)
        assert torch.equal(val, ev) and torch.equal(idx, ei) and torch.equal(pred, ep)
        hits += int((ep == label).sum())
    assert counts.tolist() == [hits, 2 * Q]


_MODELS = {}


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


@pytest.mark.parametrize("kind,metric", R.EVAL_CASES)
def test_evaluate_knn_matches_the_restatement_on_the_models_own_posteriors(kind, metric):
    model = eval_model(kind)
    g, gl, t, tl = (a.to(dev()) for a in R.eval_images(kind))
    B, k, K = R.EVAL_B, R.EVAL_K, R.EVAL_CLASSES
    batches = lambda x, y: [(x[i:i + B], y[i:i + B]) for i in range(0, x.shape[0], B)]          # noqa: E731
    res = S.evaluate_knn(model, batches(g, gl), batches(t, tl), k=k, metric=metric, weights="uniform")
    # the restatement on the model's OWN encode outputs, batched as evaluate_knn saw them
    def posterior(x):
        parts = [S.encode_posterior(model, xb) for xb, _ in batches(x, x)]
        return [torch.cat([q[j] for q in parts]).double().cpu().numpy() for j in (0, 1)]
    (mg, lg), (mq, lq) = posterior(g), posterior(t)
    decided, tol, ref = R.decided_rows(metric, mq, lq, mg, lg, k)
    print("FIG evaluate_knn %s %s undecided %d tol %.2e accuracy %.3f" % (kind, metric, int((~decided).sum()), tol, res["accuracy"]))
    assert int((~decided).sum()) <= R.MAX_UNDECIDED
    rpred = R.vote(*R.topk(ref, k, metric), gl.cpu().numpy(), K)[1]
    # per-row predictions: KnnEvaluator over the same index
    index = S.LatentIndex(mg.shape[1], metric=metric, num_classes=K)
    index.add(f32(mg), f32(lg), gl)
    ev = S.KnnEvaluator(model, index, k)
    pred = torch.cat([ev.update(x, y) for x, y in batches(t, tl)]).cpu().numpy()
    assert np.array_equal(pred[decided], rpred[decided])
    y = tl.cpu().numpy()
    for r in (res, ev.result()):
        assert r["total"] == R.EVAL_TEST and r["correct"] == int((pred == y).sum()) and r["accuracy"] == r["correct"] / r["total"]
        assert np.array_equal(r["confusion"], R.counters(pred, y, K)[1])
        rows_ = r["confusion"].sum(axis=1)
        assert np.allclose(r["per_class_accuracy"][rows_ > 0], (np.diag(r["confusion"]) / np.maximum(rows_, 1))[rows_ > 0])
    # on the decided rows the counts are the restatement's
    assert int((pred[decided] == y[decided]).sum()) == int((rpred[decided] == y[decided]).sum())
    assert np.array_equal(R.counters(pred[decided], y[decided], K)[1], R.counters(rpred[decided], y[decided], K)[1])
