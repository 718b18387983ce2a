"""The aggregate posterior on a real MI355X: sv_aggpost_sample, sv_aggpost_scan, sv_aggpost_dims and sv_aggpost_finish through the C ABI
against the float64 restatement of tests/_aggpost_ref.py (pinned to torch.distributions by tests/test_aggpost_cpu.py), then the Python
layer (shot_vae_amd.aggregate: AggregatePosterior, evaluate_aggregate).

Allowances follow the project's 8x rule and are measured when the test runs, never taken from a GPU result: 8 x the largest error of the
float32 restatement (fp32 pair values by the 16-block rule, float64 log-sum-exp, the result rounded once to fp32 as the kernels' outputs
are) against the float64 one on 64 x 64 rows of the case's recipe and dimension (A.tolerance_for; for a gallery of fewer than 64 rows
the 64 rows are cut into galleries of the case's size: a density over one row is a pair value), or on the case's own inputs for
evaluate_aggregate.  Inputs: `spread` (mu ~ N(0, 1), log sigma ~ U(-1, 0.5): one gallery row carries each sum) and `overlap` (nearly
coincident posteriors); on `overlap` at N = 130, the size the recipe is made for, each test asserts that at least 8 terms effectively
contribute (min 1 / sum w^2 on the float64 reference) -- a kernel that returned the largest term would fail there.  Smaller galleries
cannot have 8 contributing terms; they run without that condition.  States are pre-filled with garbage and carry guard elements.

Measured on an MI355X, error (allowance): scan at D = 1 9e-8 .. 1.5e-6 (8e-7 .. 1.3e-4), at D = 128 / 130 spread 2.2e-5 .. 5.6e-5 (2.1e-4 ..
6.0e-4), overlap 7.6e-6 .. 1.0e-5 (6.0e-5 .. 1.1e-4); dims at N >= 63 8e-8 .. 8.9e-7 (8e-7 .. 7.8e-6), at N = 1 1e-7 .. 1.7e-5 (4.5e-6 ..
3.3e-4); sample z 3e-7 .. 1.6e-6 (2.2e-6 .. 1.4e-5), lqx / lpz 1e-6 .. 3.7e-5 (3e-6 .. 2.2e-4), lpz - lqx against the sweep's lw 5e-7 ..
3.1e-5 (4.5e-6 .. 3.5e-4); leave-one-out 2.7e-7 .. 2.8e-5 (2e-6 .. 2.2e-4); evaluate_aggregate mi 5.6e-7 / 1.3e-7 (1.6e-4 / 4.6e-5),
total_correlation 8.4e-7 / 3.5e-7 (2.2e-3 / 6.4e-4) on wideresnet-10-1 / svhn."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import shot_vae_amd as S                                        # noqa: E402
from shot_vae_amd import _lib as L                              # noqa: E402
from shot_vae_amd import aggregate as AG                        # noqa: E402
from tests import _aggpost_ref as A                             # noqa: E402
from tests import _knn_ref as R                                 # noqa: E402

GUARD = 5
Q = 70                                                          # two query tiles of the scan (the second ragged), three of the dims
NS, DS = (1, 63, 65, 130), (1, 16, 17, 128, 130)
SCAN, DIMS = "sv_aggpost_scan", "sv_aggpost_dims"


def dev():
    return torch.device("cuda:0")


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev())


def launcher_p(name, nq, N, D):
    return AG.partials(-(-nq // 64) if name == SCAN else -(-nq // 32) * -(-D // 64), N)


def density(name, z, mu, ls, cuts=None, P=None, self0=-1, count=None):
    """the pass `name` over the gallery cut at `cuts` (row offsets; the first call has init = 1 and finds garbage in the states), then
    sv_aggpost_finish -> float64 numpy [Q] (scan) or [Q, D] (dims); the guard elements behind states and output stay as they were"""
    nq, D = z.shape
    N = mu.shape[0]
    P = P or launcher_p(name, nq, N, D)
    n_out = nq if name == SCAN else nq * D
    dz, gm, gl = f32(z), f32(mu), f32(ls)
    m = torch.full((P * n_out + GUARD,), 7.0, dtype=torch.float64, device=dev())
    s = torch.full((P * n_out + GUARD,), -3.0, dtype=torch.float64, device=dev())
    out = torch.full((n_out + GUARD,), -7.0, dtype=torch.float32, device=dev())
    edges = [0] + list(cuts or []) + [N]
    for n, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        L.call(name, p(dz), nq, p(gm[a:]), p(gl[a:]), b - a, D, a, self0, p(m), p(s), P, 1 if n == 0 else 0, st())
    L.call("sv_aggpost_finish", p(m), p(s), P, n_out, count or N, p(out), st())
    torch.cuda.synchronize()
    assert bool((m[P * n_out:] == 7.0).all()) and bool((s[P * n_out:] == -3.0).all()), name + " wrote behind its states"
    assert bool((out[n_out:] == -7.0).all()), "sv_aggpost_finish wrote behind its output"
    got = out[:n_out].double().cpu().numpy()
    return got if name == SCAN else got.reshape(nq, D)


def reference(name, z, mu, ls, **kw):
    return (A.log_density if name == SCAN else A.log_density_dims)(z, mu, ls, **kw)


def tol_of(name, recipe, D, N=64):
    return A.tolerance_for("scan" if name == SCAN else "dims", recipe, D, N)


def case(recipe, N, D):
    mu, ls = A.rows(recipe, N, D, 9801)
    z = A.queries(recipe, Q, D, 9803)
    if recipe == "overlap" and N == 130:
        assert A.min_ess(z, mu, ls) >= A.MIN_ESS
    return z, mu, ls


# ================================================================================================ sv_aggpost_sample
def sample(mu, ls, key, row0, s):
    nq, D = mu.shape
    dm, dl = f32(mu), f32(ls)
    dk = None if key is None else torch.tensor([key], dtype=torch.int64, device=dev())
    z = torch.full((nq + GUARD, D), -7.0, dtype=torch.float32, device=dev())
    lqx = torch.full((nq + GUARD,), -7.0, dtype=torch.float32, device=dev())
    lpz = torch.full((nq + GUARD,), -7.0, dtype=torch.float32, device=dev())
    L.call("sv_aggpost_sample", p(dm), p(dl), p(dk), row0, s, nq, D, p(z), p(lqx), p(lpz), st())
    torch.cuda.synchronize()
    assert all(bool((t[nq:] == -7.0).all()) for t in (z, lqx, lpz)), "sv_aggpost_sample wrote behind its outputs"
    return z[:nq].clone(), lqx[:nq].clone(), lpz[:nq].clone()


@pytest.mark.parametrize("recipe", A.RECIPES)
@pytest.mark.parametrize("D", DS + (261,))
def test_sample_matches_the_restatement_and_the_sweep(recipe, D):
    mu, ls = A.rows(recipe, Q, D, 9805)
    key, row0, s = 0x1234567890, 2 ** 33 + 5, 3
    z, lqx, lpz = sample(mu, ls, key, row0, s)
    rz, rqx, rpz = A.sample(mu, ls, key, row0, s)
    tz, tqx, tpz = A.tolerance_for("sample", recipe, D)
    errs = [float(np.abs(a.double().cpu().numpy() - b).max()) for a, b in ((z, rz), (lqx, rqx), (lpz, rpz))]
    print("FIG sample %s D=%d err z %.2e (%.2e) lqx %.2e (%.2e) lpz %.2e (%.2e)" % (recipe, D, errs[0], tz, errs[1], tqx, errs[2], tpz))
    assert errs[0] <= tz and errs[1] <= tqx and errs[2] <= tpz
    # the stream of sv_latent_sweep: the fp32 latent of sample s of a sweep of S = s + 1 samples, bit for bit, and its lw
    B, Sn = Q, s + 1
    lat = torch.full((B * Sn, D + 1), -7.0, dtype=torch.float32, device=dev())
    lw = torch.full((B, Sn), -7.0, dtype=torch.float32, device=dev())
    dm, dl = f32(mu), f32(ls)
    dk = torch.tensor([key], dtype=torch.int64, device=dev())
    lab = torch.zeros(B, dtype=torch.int64, device=dev())
    L.call("sv_latent_sweep", L.SV_F32, p(dm), p(dl), p(dk), row0, p(lab), B, Sn, 1, D, D + 1, 0, B * Sn, p(lat), p(lw), st())
    torch.cuda.synchronize()
    assert torch.equal(lat.view(B, Sn, D + 1)[:, s, :D], z)
    err = float((lpz.double() - lqx.double() - lw[:, s].double()).abs().max())
    print("FIG sample lw err %.2e (%.2e)" % (err, tqx + tpz))
    assert err <= tqx + tpz
    # key = NULL: z = mu bit for bit; rows drawn in two calls equal one call bit for bit
    z0, lqx0, _ = sample(mu, ls, None, row0, s)
    assert torch.equal(z0, f32(mu))
    assert float(np.abs(lqx0.double().cpu().numpy() - A.sample(mu, ls, None, row0, s)[1]).max()) <= tqx
    a, b = sample(mu[:33], ls[:33], key, row0, s), sample(mu[33:], ls[33:], key, row0 + 33, s)
    for one, x, y in zip((z, lqx, lpz), a, b):
        assert torch.equal(one, torch.cat([x, y]))


# ================================================================================================ sv_aggpost_scan / dims / finish
@pytest.mark.parametrize("recipe", A.RECIPES)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("D", DS)
def test_density_matches_float64(recipe, N, D):
    z, mu, ls = case(recipe, N, D)
    for name in (SCAN, DIMS):
        ref, tol = reference(name, z, mu, ls), tol_of(name, recipe, D, N)
        got = density(name, z, mu, ls)
        err = float(np.abs(got - ref).max())
        print("FIG %s %s N=%d D=%d P=%d err %.3e tol %.3e" % (name, recipe, N, D, launcher_p(name, Q, N, D), err, tol))
        assert err <= tol
        # P = 1 and the launcher's own P agree; a repeat gives the same bits
        one = density(name, z, mu, ls, P=1)
        assert float(np.abs(one - ref).max()) <= tol and float(np.abs(one - got).max()) <= tol
        assert np.array_equal(got, density(name, z, mu, ls))
    if D == 1:                                             # one dimension: the marginal IS the joint
        assert float(np.abs(density(DIMS, z, mu, ls)[:, 0] - density(SCAN, z, mu, ls)).max()) <= tol_of(SCAN, recipe, 1, N) + tol_of(DIMS, recipe, 1, N)


@pytest.mark.parametrize("recipe", A.RECIPES)
@pytest.mark.parametrize("D", (17, 130))
def test_gallery_cuts_agree(recipe, D):
    """one call, 1 + 64 + 65 with col0, and 13 x 10"""
    z, mu, ls = case(recipe, 130, D)
    for name in (SCAN, DIMS):
        ref, tol = reference(name, z, mu, ls), tol_of(name, recipe, D)
        one = density(name, z, mu, ls)
        for cuts in ([1, 65], list(range(10, 130, 10))):
            for P in (None, 1, 5):
                got = density(name, z, mu, ls, cuts=cuts, P=P)
                assert float(np.abs(got - ref).max()) <= tol and float(np.abs(got - one).max()) <= tol, (name, cuts, P)
                assert np.array_equal(got, density(name, z, mu, ls, cuts=cuts, P=P))


@pytest.mark.parametrize("recipe", A.RECIPES)
@pytest.mark.parametrize("D", (16, 130))
def test_leave_one_out(recipe, D):
    """the queries are draws from gallery rows 30 .. 99: with self0 = 30 row 30 + i is left out of query i's sum, count = N - 1"""
    N, off = 130, 30
    mu, ls = A.rows(recipe, N, D, 9801)
    z = A.sample(mu[off:off + Q], ls[off:off + Q], 21, off, 0, np.float32)[0].astype(np.float64)
    for name in (SCAN, DIMS):
        ref, tol = reference(name, z, mu, ls, self0=off, count=N - 1), tol_of(name, recipe, D)
        full = reference(name, z, mu, ls)
        assert float(np.abs(ref - full).max()) > 4.0 * tol, "the case does not see the exclusion"
        for cuts in (None, [off], [64, 100]):
            got = density(name, z, mu, ls, cuts=cuts, self0=off, count=N - 1)
            err = float(np.abs(got - ref).max())
            print("FIG loo %s %s D=%d cuts %s err %.3e tol %.3e" % (name, recipe, D, cuts, err, tol))
            assert err <= tol


def test_special_values():
    N, D = 70, 17
    z, mu, ls = case("overlap", N, D)
    z, mu, ls = z[:9].copy(), mu.copy(), ls.copy()
    # a gallery row with ls = +inf has weight 0: the sum of the others, over the same count
    ls_inf = ls.copy()
    ls_inf[66] = np.inf
    keep = np.arange(N) != 66
    for name in (SCAN, DIMS):
        tol = tol_of(name, "overlap", D)
        got = density(name, z, mu, ls_inf, cuts=[64])
        assert float(np.abs(got - reference(name, z, mu[keep], ls[keep], count=N)).max()) <= tol
        # a query for which every term is -inf gives -inf (not NaN); its neighbours are untouched
        zi = z.copy()
        zi[4] = np.inf
        got = density(name, zi, mu, ls)
        assert (got[4] == -np.inf).all()
        assert float(np.abs(np.delete(got, 4, 0) - np.delete(reference(name, z, mu, ls), 4, 0)).max()) <= tol
        # a NaN gallery row makes every query NaN; a NaN query row only itself
        mu_nan = mu.copy()
        mu_nan[65] = np.nan
        for P in (None, 1):
            assert np.isnan(density(name, z, mu_nan, ls, P=P)).all()
        assert np.isnan(density(name, z, mu_nan, ls, cuts=[3, 64])).all()
        zn = z.copy()
        zn[2] = np.nan
        got = density(name, zn, mu, ls)
        assert np.isnan(got[2]).all() and np.isfinite(np.delete(got, 2, 0)).all()
        assert float(np.abs(np.delete(got, 2, 0) - np.delete(reference(name, z, mu, ls), 2, 0)).max()) <= tol


@pytest.mark.parametrize("D", (17, 128))
def test_identical_gallery_rows_give_the_single_value(D):
    mu1, ls1 = A.rows("spread", 1, D, 9807)
    z = A.queries("overlap", Q, D, 9803)
    mu, ls = np.repeat(mu1, 130, axis=0), np.repeat(ls1, 130, axis=0)
    got = density(SCAN, z, mu, ls)
    assert float(np.abs(got - A.pair_values(z, mu1, ls1)[:, 0]).max()) <= A.tolerance_for("pair", "spread", D)
    got = density(DIMS, z, mu, ls)
    assert float(np.abs(got - A.dim_values(z, mu1, ls1)[:, 0, :]).max()) <= A.tolerance_for("dims", "spread", D, 1)


# ================================================================================================ the Python layer
def test_aggregate_posterior_added_in_pieces_equals_added_at_once():
    N, D = 1500, 17                                         # 1500 rows: the buffers grow once on the way (1024 -> 2048)
    mu, ls = A.rows("overlap", N, D, 9809)
    z = f32(A.queries("overlap", Q, D, 9803))
    gm, gl = f32(mu), f32(ls)
    one = S.AggregatePosterior(D)
    assert one.add(gm, gl) == 0 and len(one) == N
    three = S.AggregatePosterior(D)
    assert [three.add(gm[a:b], gl[a:b]) for a, b in ((0, 700), (700, 1200), (1200, N))] == [0, 700, 1200] and len(three) == N
    a, b = one.log_density(z, per_dim=True), three.log_density(z, per_dim=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], one.log_density(z))
    assert tuple(a[0].shape) == (Q,) and tuple(a[1].shape) == (Q, D) and a[0].dtype == a[1].dtype == torch.float32
    zz = z.double().cpu().numpy()
    assert float(np.abs(a[0].double().cpu().numpy() - A.log_density(zz, mu, ls)).max()) <= A.tolerance_for("scan", "overlap", D)
    assert float(np.abs(a[1].double().cpu().numpy() - A.log_density_dims(zz, mu, ls)).max()) <= A.tolerance_for("dims", "overlap", D)
    # sample() is sv_aggpost_sample; leave-one-out through the object: draws from the gallery's own rows 700 .. 769
    zs, lqx, lpz = one.sample(gm[700:700 + Q], gl[700:700 + Q], key=21, row0=700, s=1)
    rz, rqx, rpz = A.sample(mu[700:700 + Q], ls[700:700 + Q], 21, 700, 1)
    tz, tqx, tpz = A.tolerance_for("sample", "overlap", D)
    assert float(np.abs(zs.double().cpu().numpy() - rz).max()) <= tz and float(np.abs(lqx.double().cpu().numpy() - rqx).max()) <= tqx
    assert float(np.abs(lpz.double().cpu().numpy() - rpz).max()) <= tpz
    loo = one.log_density(zs, exclude_self_from=700)
    ref = A.log_density(zs.double().cpu().numpy(), mu, ls, self0=700, count=N - 1)
    assert float(np.abs(loo.double().cpu().numpy() - ref).max()) <= A.tolerance_for("scan", "overlap", D)
    # shape errors are ValueErrors, raised before any call into the library
    for fn in (lambda: one.log_density(z[:, :5]), lambda: one.log_density(z.view(-1)), lambda: one.sample(gm[:, :5], gl[:, :5]),
               lambda: one.sample(gm[:4], gl[:3]), lambda: one.add(gm[:, :5], gl[:, :5]), lambda: one.log_density(z, exclude_self_from=-2),
               lambda: one.sample(gm[:4], gl[:4], key=1, s=65536), lambda: one.sample(gm[:4], gl[:4], key=1, row0=-1),
               lambda: S.AggregatePosterior(D).log_density(z)):
        with pytest.raises(ValueError):
            fn()


def test_log_density_under_graph_capture():
    N, D = 300, 128
    mu, ls = A.rows("overlap", N, D, 9809)
    agg = S.AggregatePosterior(D)
    agg.add(f32(mu), f32(ls))
    zs = [f32(A.queries("overlap", Q, D, s)) for s in (9811, 9813)]
    sz = zs[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                           # warm-up outside the capture
        agg.log_density(sz, per_dim=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lq, lqd = agg.log_density(sz, per_dim=True)
    for z in (zs[1], zs[0]):                                # replayed on new z
        sz.copy_(z)
        graph.replay()
        torch.cuda.synchronize()
        e = agg.log_density(z, per_dim=True)
        assert torch.equal(lq, e[0]) and torch.equal(lqd, e[1])
    assert not torch.equal(agg.log_density(zs[0]), agg.log_density(zs[1]))


# ================================================================================================ evaluate_aggregate
_MODELS = {}
EVAL_N, EVAL_B = 96, 16


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


@pytest.mark.parametrize("kind", R.EVAL_KINDS)
def test_evaluate_aggregate_matches_the_restatement_on_the_models_own_posteriors(kind):
    model = eval_model(kind)
    x = R.eval_images(kind)[0].to(dev())
    assert x.shape[0] == EVAL_N
    batches = lambda b: [x[i:i + b] for i in range(0, EVAL_N, b)]          # noqa: E731
    samples, key = 2, 31
    res = S.evaluate_aggregate(model, batches(EVAL_B), samples=samples, key=key)
    # the restatement on the model's OWN encode outputs, batched as evaluate_aggregate saw them
    parts = [S.encode_posterior(model, xb) for xb in batches(EVAL_B)]
    mu, ls = (torch.cat([q[j] for q in parts]).double().cpu().numpy() for j in (0, 1))
    third = torch.cat([model.encode(xb)[2].detach() for xb in batches(EVAL_B)]).double()
    qy = (third if kind == "svhn" else torch.exp(third)).cpu().numpy()
    D = mu.shape[1]
    ref = A.diagnostics(mu, ls, qy, samples=samples, key=key)
    # allowances: 8 x the float32 restatement's error per OUTPUT on these inputs, then the number of terms each diagnostic adds up
    e = dict(lqx=0.0, lq=0.0, lpz=0.0, lqd=0.0, hz2=0.0)
    for s in range(samples):
        (z32, a32, c32), (z64, a64, c64) = A.sample(mu, ls, key, 0, s, np.float32), A.sample(mu, ls, key, 0, s)
        z32 = z32.astype(np.float64)
        for name, got, want in (("lqx", a32, a64), ("lpz", c32, c64), ("lq", A.log_density(z32, mu, ls, np.float32), A.log_density(z64, mu, ls)),
                                ("lqd", A.log_density_dims(z32, mu, ls, np.float32), A.log_density_dims(z64, mu, ls)),
                                ("hz2", 0.5 * z32 * z32, 0.5 * z64 * z64)):
            e[name] = max(e[name], 8.0 * float(np.abs(got - want).max()))
    tol = dict(mi=e["lqx"] + e["lq"], marginal_kl=e["lq"] + e["lpz"], kl_c_mc=e["lqx"] + e["lpz"], total_correlation=e["lq"] + D * e["lqd"],
               dimwise_kl=D * (e["lqd"] + e["hz2"]), kl_c=1e-9 * max(1.0, ref["kl_c"]), mi_y=1e-9, marginal_kl_y=1e-9)
    for k, t in tol.items():
        print("FIG evaluate_aggregate %s %-17s got %.6e ref %.6e err %.2e tol %.2e" % (kind, k, res[k], ref[k], abs(res[k] - ref[k]), t))
    for k, t in tol.items():
        assert abs(res[k] - ref[k]) <= t, k
    assert res["dim_kl"].shape == (D,) and float(np.abs(res["dim_kl"] - ref["dim_kl"]).max()) <= e["lqd"] + e["hz2"]
    assert res["active_units"] == ref["active_units"] and abs(res["log_n"] - np.log(EVAL_N)) <= 1e-15 and abs(ref["log_n"] - np.log(EVAL_N)) <= 1e-15
    assert set(res) == set(ref)
    # the identities, and the ceiling
    assert abs(res["mi"] + res["marginal_kl"] - res["kl_c_mc"]) <= 4.0 * np.finfo(np.float32).eps * max(1.0, abs(res["kl_c_mc"]))
    assert res["mi"] <= res["log_n"] + tol["mi"]
    # re-batched: 96 = 6 x 16 = 2 x 48
    again = S.evaluate_aggregate(model, batches(48), samples=samples, key=key)
    for k, t in tol.items():
        assert abs(again[k] - res[k]) <= t + (1e-6 * max(1.0, abs(res[k])) if k in ("kl_c", "mi_y", "marginal_kl_y") else 0.0), k
    # without the per-dimension pass, and with the queries given: the same numbers
    lean = S.evaluate_aggregate(model, batches(EVAL_B), samples=samples, key=key, per_dim=False, query_batches=batches(EVAL_B))
    assert "dim_kl" not in lean and "total_correlation" not in lean and "dimwise_kl" not in lean
    for k in ("mi", "marginal_kl", "kl_c_mc"):
        assert abs(lean[k] - res[k]) <= tol[k]
