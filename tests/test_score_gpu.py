"""Per-image scores on a real MI355X: sv_latent_sweep, sv_recon_rows and sv_score_reduce through the C ABI, and score / log_likelihood /
evaluate_scores of the model.

Kernel level: against the float64 numpy restatements of tests/_score_ref.py (written from the header comments).  Exact quantities
-- the class part, the pad columns, every bit-for-bit property, the positions of infinities -- are compared exactly; the others by the
house rule of tests/test_head_loss_kernels_gpu.py: the kernel gets 8 x the error of an fp32 numpy restatement against the float64 one
(at least 8 x 2^-24), max |a - ref| / max |ref| over the tensor, measured on the test's own inputs.  Outputs are NaN-prefilled and
carry guard tails.  Measured on an MI355X (cpu32 = the fp32 restatement, kernel, allowance = 8 x max(cpu32, 2^-24)):
    sv_latent_sweep  z   (f32 / bf16 latent; all of ldc, K, S, B)   cpu32 <= 2.8e-7   kernel <= 2.8e-7   allowance 4.8e-7 .. 2.2e-6
    sv_latent_sweep  lw                                             cpu32 <= 1.6e-7   kernel <= 1.2e-7   allowance 4.8e-7 .. 1.3e-6
    sv_latent_sweep  lw, no key                                     cpu32 <= 9.5e-8   kernel <= 4.5e-8   allowance 4.8e-7 .. 7.6e-7
    sv_recon_rows    BCE (f32 / bf16 logits; all of C, R, rpi)      cpu32 <= 1.4e-7   kernel <= 5.5e-8   allowance 4.8e-7 .. 1.1e-6
    sv_recon_rows    MSE, x_sigma = 0.5                             cpu32 <= 9.8e-8   kernel <= 4.7e-8   allowance 4.8e-7 .. 7.9e-7
    sv_score_reduce  recon / kl_c / kl_d / elbo / log_px            cpu32 <= 2.2e-7   kernel <= 5.2e-8   allowance 4.8e-7 .. 1.8e-6

Model level, fp32-operand mode against the reference's fixture (tests/golden/make_score_goldens.py): relative <= 1e-3 per image, the
project's fp32 gate.  (The closed-form decoder depends on its input only weakly -- the fixture's terms differ by ~1e-6 between classes
-- so that gate does not tell the classes apart; the wiring of classes and samples is held by the kernel tests' exact comparisons of
the one-hot block and of the row-to-image map.)  Ties to the existing path: score against VAECriterion on decode(), evaluate_scores
against its own re-batching, chunked against unchunked, preactresnet18.  bf16 against fp32 at the project's 5e-3 gate on loss scalars,
and log_likelihood under graph capture."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import shot_vae_amd as S                                        # noqa: E402
from shot_vae_amd import _lib as L                              # noqa: E402
from oracle import closed_form as CF                            # noqa: E402
from tests import _cases as T                                   # noqa: E402
from tests.golden import make_score_goldens as G                # noqa: E402
from tests.test_infer_gpu import DT, GUARD, HALF_ULP, NAN, bf16_round, close, dev, dev_t, infer_model, p, rel, st      # noqa: E402
from tests.test_model_gpu import FP32_TOL, make_model           # noqa: E402
from tests._score_ref import nll_rows, ref_scores, sweep_lw, sweep_z        # noqa: E402

BF16_TOL = 5e-3          # bf16 operands, loss scalars


# ================================================================================================ sv_latent_sweep
def sweep(dt, B, S_, K, ldc, Lpad, mu, ls, key, row0=0, label=None, j0=0, R=None, lw=None):
    """one sv_latent_sweep call into a NaN-filled latent with guard rows -> (latent [R, Lpad] float64 numpy, lw [B, S] fp32 numpy).  `lw`:
    a device buffer to write into (the caller's chunks share one), else a fresh NaN-filled one with a guard tail."""
    code, tt = DT[dt]
    Kd = 1 if label is not None else K
    R = B * S_ * Kd - j0 if R is None else R
    latent = torch.full((R + GUARD, Lpad), NAN, dtype=tt, device=dev())
    own = lw is None
    if own:
        lw = torch.full((B * S_ + GUARD,), NAN, dtype=torch.float32, device=dev())
    L.call("sv_latent_sweep", code, p(mu), p(ls), p(key), int(row0), p(label), B, S_, K, ldc, Lpad, j0, R, p(latent), p(lw), st())
    torch.cuda.synchronize()
    assert torch.isnan(latent[R:].float()).all(), "guard rows written"
    assert not own or torch.isnan(lw[B * S_:]).all(), "lw guard written"
    return latent[:R].double().cpu().numpy(), lw[:B * S_].cpu().numpy().reshape(B, S_)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("ldc", [5, 128])
@pytest.mark.parametrize("K", [1, 10, 100])
def test_latent_sweep_against_float64(dt, ldc, K):
    keyv = 0x0123456789ABCDEF
    key = torch.tensor([keyv], dtype=torch.int64, device=dev())
    Lpad = (ldc + K + 15) // 16 * 16 + 16
    exact = (lambda a: a) if dt == "f32" else bf16_round
    for B in (1, 7):
        for S_ in (1, 3):
            row0 = 2 ** 32 - 3 if (B, S_) == (7, 3) else 11           # the rows cross 2^32, the second counter word
            rng = np.random.default_rng(100 * ldc + 10 * K + B + S_)
            mu = (rng.standard_normal((B, ldc)) * 0.7).astype(np.float32)
            ls = (rng.standard_normal((B, ldc)) * 0.3 - 0.5).astype(np.float32)
            label = ((np.arange(B) * 7 + 3) % K).astype(np.int64)
            label[0] = K                                              # out of range: no class
            if B > 2:
                label[2] = -1
            d_mu, d_ls, d_label = dev_t(mu), dev_t(ls), dev_t(label)
            tag = "latent_sweep %s ldc=%d K=%d B=%d S=%d" % (dt, ldc, K, B, S_)
            z64, z32 = sweep_z(keyv, row0, B, S_, ldc, mu, ls), sweep_z(keyv, row0, B, S_, ldc, mu, ls, np.float32)
            lw64, lw32 = sweep_lw(keyv, row0, B, S_, ldc, mu, ls), sweep_lw(keyv, row0, B, S_, ldc, mu, ls, np.float32)
            # --- the class sweep: row (b, s, k) = [z_{b,s} | onehot k | 0]
            zf, _ = sweep("f32", B, S_, K, ldc, Lpad, d_mu, d_ls, key, row0)       # the fp32 z, whatever the dtype under test
            zf = zf[:, :ldc].reshape(B, S_, K, ldc)
            lat, lw = sweep(dt, B, S_, K, ldc, Lpad, d_mu, d_ls, key, row0)
            lat4 = lat.reshape(B, S_, K, Lpad)
            close(zf[:, :, 0], z32, z64, tag + " z")
            close(lw, lw32, lw64, tag + " lw")
            assert np.array_equal(lat4[..., :ldc], exact(zf)), "the latent's z part is not the rounding of the fp32 z"
            assert all(np.array_equal(zf[:, :, k], zf[:, :, 0]) for k in range(K)), "the class rows of one sample share z"
            assert np.array_equal(lat4[..., ldc:ldc + K], np.broadcast_to(np.eye(K), (B, S_, K, K))), "one-hot block of row (b, s, k)"
            assert np.all(lat4[..., ldc + K:] == 0.0), "pad columns"
            # --- label mode: one row per sample
            onehot = np.zeros((B, K))
            for b in range(B):
                if 0 <= label[b] < K:
                    onehot[b, label[b]] = 1.0
            latl, lwl = sweep(dt, B, S_, K, ldc, Lpad, d_mu, d_ls, key, row0, label=d_label)
            latl = latl.reshape(B, S_, Lpad)
            assert np.array_equal(latl[..., :ldc], lat4[:, :, 0, :ldc]) and np.array_equal(lwl, lw)
            assert np.array_equal(latl[..., ldc:ldc + K], np.broadcast_to(onehot[:, None], (B, S_, K))) and np.all(latl[..., ldc + K:] == 0.0)
            # --- no key: z == mu bit for bit
            if S_ == 1:
                lat0, lw0 = sweep(dt, B, 1, K, ldc, Lpad, d_mu, d_ls, None, row0)
                assert np.array_equal(lat0.reshape(B, K, Lpad)[:, :, :ldc], np.broadcast_to(exact(mu)[:, None], (B, K, ldc))), "null key: z == mu"
                close(lw0, sweep_lw(None, 0, B, 1, ldc, mu, ls, np.float32), sweep_lw(None, 0, B, 1, ldc, mu, ls), tag + " lw, no key")
            # --- rows drawn in two calls (row0) equal the rows drawn in one, bit for bit; so does any chunk (j0, R) of the sweep
            if B > 1:
                b1 = 3
                la_, lwa = sweep(dt, b1, S_, K, ldc, Lpad, d_mu[:b1], d_ls[:b1], key, row0)
                lb_, lwb = sweep(dt, B - b1, S_, K, ldc, Lpad, d_mu[b1:], d_ls[b1:], key, row0 + b1)
                assert np.array_equal(np.concatenate([la_, lb_]), lat) and np.array_equal(np.concatenate([lwa, lwb]), lw)
                total = B * S_ * K
                cuts = [0, total // 3 + 1, total - 2, total]
                shared = torch.full((B * S_,), NAN, dtype=torch.float32, device=dev())
                parts = [sweep(dt, B, S_, K, ldc, Lpad, d_mu, d_ls, key, row0, j0=a, R=b - a, lw=shared)[0] for a, b in zip(cuts, cuts[1:]) if b > a]
                assert np.array_equal(np.concatenate(parts), lat), "chunks of the sweep differ from the whole"
                assert np.array_equal(shared.cpu().numpy().reshape(B, S_), lw), "lw written by chunks differs"
    # --- the key is read on the device
    key.fill_(keyv + 1)
    lat_b, _ = sweep(dt, B, S_, K, ldc, Lpad, d_mu, d_ls, key, row0)
    assert float(np.mean(lat_b.reshape(B, S_, K, Lpad)[..., :ldc] != lat4[..., :ldc])) > 0.95


# ================================================================================================ sv_recon_rows
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("Cc", [1, 3])
@pytest.mark.parametrize("R,rpi", [(1, 1), (7, 1), (130, 1), (1, 30), (7, 30), (130, 30)])
def test_recon_rows_against_float64(dt, Cc, R, rpi):
    code, tt = DT[dt]
    H = W = 32
    ld = 16
    B = (R - 1) // rpi + 1
    rng = np.random.default_rng(7 + R + rpi + Cc)
    r = torch.from_numpy((rng.standard_normal((R, H, W, ld)) * 3.0).astype(np.float32))
    r[0, 0, :6, 0] = torch.tensor([80.0, -80.0, 0.0, -0.0, 30.0, -30.0])
    r[R - 1, 5, :2, Cc - 1] = torch.tensor([-80.0, 80.0])
    r = r.to(tt).float().numpy()                       # the values the kernel reads, exact in either dtype
    x = rng.random((B, Cc, H, W)).astype(np.float32)
    x[0, 0, 0, :6] = [0.0, 1.0, 1.0, 0.0, 1.0, 0.0]    # the +-80 logits meet pixels 0 and 1, matching and not
    x[B - 1, Cc - 1, 5, :2] = [1.0, 0.0]
    d_r, d_x = dev_t(r, tt), dev_t(x)
    rows = np.transpose(r[..., :Cc], (0, 3, 1, 2))
    xr = x[np.arange(R) // rpi]

    def run(bce, sig, j0=0, n=R):
        nll = torch.full((n + GUARD,), NAN, dtype=torch.float32, device=dev())
        L.call("sv_recon_rows", code, C.c_void_p(d_r.data_ptr() + j0 * H * W * ld * d_r.element_size()), p(d_x), B, j0, n, rpi, Cc, H, W, ld,
               bce, sig, p(nll), st())
        torch.cuda.synchronize()
        assert torch.isnan(nll[n:]).all(), "guard tail written"
        return nll[:n].cpu().numpy()

    for bce, sig in ((1, 1.0), (0, 0.5)):
        tag = "recon_rows %s C=%d R=%d rpi=%d %s" % (dt, Cc, R, rpi, "bce" if bce else "mse")
        got = run(bce, sig)
        close(got, nll_rows(rows, xr, bce, sig, np.float32), nll_rows(rows, xr, bce, sig), tag)
        assert np.array_equal(got, run(bce, sig)), "two launches differ"
        if R > 2:                                      # a chunk of the rows: the image of row j0 + j
            j0 = R // 2 + 1
            assert np.array_equal(run(bce, sig, j0, R - j0), got[j0:]), "a chunk differs from the whole"


# ================================================================================================ sv_score_reduce
NAMES = ("recon", "kl_c", "kl_d", "elbo", "log_px")


def reduce_call(nll, lw, la, mu, ls, add, want):
    B, S_, Kd = nll.shape
    out = {w: torch.full((B + GUARD,), NAN, dtype=torch.float32, device=dev()) for w in want}
    L.call("sv_score_reduce", p(nll), p(lw), p(la), p(mu), p(ls), B, S_, Kd, la.shape[1], mu.shape[1], float(add),
           *[p(out.get(w)) for w in NAMES], st())
    torch.cuda.synchronize()
    assert all(torch.isnan(v[B:]).all() for v in out.values()), "guard tail written"
    return {w: v[:B].cpu().numpy() for w, v in out.items()}


def close_with_inf(got, f32, ref, what):
    """`close` on the finite entries; the infinite ones must sit where the reference's do, with its sign; no NaN anywhere"""
    assert not np.isnan(got).any(), what + ": NaN"
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin].astype(np.float32)), what + ": infinities differ"
    if fin.any():
        close(got[fin], f32[fin], ref[fin], what)


@pytest.mark.parametrize("S_", [1, 3, 64])
@pytest.mark.parametrize("Kd", [1, 10, 100])
def test_score_reduce_against_float64(S_, Kd):
    K = 10 if Kd == 1 else Kd
    B, ldc = 6, 37
    for scale in (1.0, 1.0e4):
        rng = np.random.default_rng(S_ + Kd)
        nll = (scale + 3.0 * rng.random((B, S_, Kd))).astype(np.float32)
        lw = (rng.standard_normal((B, S_)) * 4.0 - 20.0).astype(np.float32)
        la = np.log(rng.dirichlet(np.ones(K), size=B)).astype(np.float32)
        mu = (rng.standard_normal((B, ldc)) * 0.7).astype(np.float32)
        ls = (rng.standard_normal((B, ldc)) * 0.3 - 0.5).astype(np.float32)
        if S_ * Kd > 1:
            nll[1, 0, 0] = np.inf                              # one +inf term: weight 0 in log_px
        nll[2] = np.inf                                        # every term +inf: log_px = -inf, not NaN
        if K > 1:                                              # classes of probability 0, one of them with an infinite term
            la[3, [0, K - 1]] = -np.inf
            la[3] -= np.log(np.exp(la[3].astype(np.float64)).sum()).astype(np.float32)
            if Kd > 1:
                nll[3, :, 0] = np.inf
        if S_ > 1:
            lw[4, 1] = -np.inf                                 # a sample of weight 0
        add = -1234.5
        ref = ref_scores(nll, lw, la, mu, ls, add)
        with np.errstate(over="ignore", invalid="ignore"):
            f32 = ref_scores(nll, lw, la, mu, ls, add, np.float32)
        assert ref["log_px"][2] == -np.inf and np.isfinite(ref["log_px"][[0, 1, 3, 5]]).all() and np.isfinite(ref["recon"][3])
        d = [dev_t(v) for v in (nll, lw, la, mu, ls)]
        tag = "score_reduce S=%d Kd=%d scale=%g " % (S_, Kd, scale)
        both = reduce_call(*d, add, NAMES)
        for w in NAMES:
            close_with_inf(both[w], f32[w], ref[w], tag + w)
            alone = reduce_call(*d, add, (w,))
            assert np.array_equal(alone[w], both[w], equal_nan=True), "%s alone differs from all five together" % w
        again = reduce_call(*d, add, NAMES)
        assert all(np.array_equal(again[w], both[w]) for w in NAMES), "two launches differ"
        no_lw = reduce_call(d[0], None, *d[2:], add, NAMES[:4])         # lw is optional without log_px
        assert all(np.array_equal(no_lw[w], both[w]) for w in NAMES[:4])


def test_score_reduce_propagates_nan():
    """a NaN in nll, lw or la is never dropped: every output it enters is NaN, the other images' outputs are untouched"""
    B, S_, K, ldc = 5, 3, 4, 8
    rng = np.random.default_rng(3)
    nll = (5.0 + rng.random((B, S_, K))).astype(np.float32)
    lw = rng.standard_normal((B, S_)).astype(np.float32)
    la = np.log(rng.dirichlet(np.ones(K), size=B)).astype(np.float32)
    mu, ls = rng.standard_normal((B, ldc)).astype(np.float32), (rng.standard_normal((B, ldc)) * 0.3).astype(np.float32)
    clean = reduce_call(*[dev_t(v) for v in (nll, lw, la, mu, ls)], 0.0, NAMES)
    nll[0, 1, 2] = np.nan
    nll[1, 0, 0], nll[1, 2, 1] = np.inf, np.nan                 # behind a running maximum of -inf
    lw[2, 1] = np.nan
    la[3, 1] = np.nan
    got = reduce_call(*[dev_t(v) for v in (nll, lw, la, mu, ls)], 0.0, NAMES)
    with np.errstate(invalid="ignore"):
        ref = ref_scores(nll, lw, la, mu, ls)
    for w in NAMES:
        assert np.array_equal(np.isnan(got[w]), np.isnan(ref[w])), (w, got[w], ref[w])
        assert np.array_equal(got[w][4:], clean[w][4:])
    assert np.isnan(got["log_px"][:3]).all() and np.isnan(got["recon"][[0, 1, 3]]).all() and np.isnan(got["kl_d"][3])
    assert not np.isnan(got["recon"][2]) and not np.isnan(got["kl_c"]).any() and not np.isnan(got["log_px"][3])


# ================================================================================================ model level
def per_image(got, ref):
    """max over the images of |got - ref| / |ref|"""
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    return float((np.abs(got - ref) / np.abs(ref)).max())


def crits():
    return {"bce": S.VAECriterion(discrete_dim=G.K, x_sigma=1, bce_reconstruction=True),
            "mse": S.VAECriterion(discrete_dim=G.K, x_sigma=G.X_SIGMA, bce_reconstruction=False)}


def gate(what, got, ref, tol=FP32_TOL):
    e = per_image(got, ref)
    print("FIG %-46s %.3e" % (what, e))
    assert e <= tol, (what, e)


def test_score_at_the_posterior_mean_matches_the_reference():
    g = T.load(G.TAG)
    model, _ = infer_model(G.NAME)
    x = G.score_inputs().cuda()
    q = np.exp(g["la"].astype(np.float64))
    for mode, crit in crits().items():
        for k in range(G.K):
            sc = model.score(x, crit, label=torch.full((G.B,), k, dtype=torch.int64, device="cuda"))
            assert isinstance(sc, S.Scores) and all(t.shape == (G.B,) and t.dtype == torch.float32 and not t.requires_grad for t in sc)
            gate("score %s label=%d recon" % (mode, k), sc.recon, g["nll_mu_" + mode][:, k])
            gate("score %s label=%d kl_c" % (mode, k), sc.kl_c, g["kl_c"])
            gate("score %s label=%d kl_d" % (mode, k), sc.kl_d, g["kl_d"])
            gate("score %s label=%d elbo" % (mode, k), sc.elbo, -(g["nll_mu_" + mode][:, k].astype(np.float64) + g["kl_c"] + g["kl_d"]))
        sc = model.score(x, crit)
        want = (q * g["nll_mu_" + mode]).sum(axis=1)
        gate("score %s label=None recon" % mode, sc.recon, want)
        gate("score %s label=None elbo" % mode, sc.elbo, -(want + g["kl_c"] + g["kl_d"]))


def test_sampled_score_and_log_likelihood_match_the_reference():
    g = T.load(G.TAG)
    model, _ = infer_model(G.NAME)
    x = G.score_inputs().cuda()
    key = torch.tensor([G.KEY], dtype=torch.int64, device="cuda")
    mu, ls, z = (g[k].astype(np.float64) for k in ("mu", "ls", "z"))
    n = (z - mu[:, None]) / np.exp(ls)[:, None]
    lw = (0.5 * n * n - 0.5 * z * z + ls[:, None]).sum(axis=2)                    # from the recorded z
    # the kernel's z on the recorded mu / ls is the recorded z, to the stream's allowance
    Lpad = model._plan.Lpad
    lat, _ = sweep("f32", G.B, G.S, G.K, G.LDC, Lpad, dev_t(g["mu"]), dev_t(g["ls"]), key, G.ROW0)
    close(lat.reshape(G.B, G.S, G.K, Lpad)[:, :, 0, :G.LDC], sweep_z(G.KEY, G.ROW0, G.B, G.S, G.LDC, g["mu"], g["ls"], np.float32),
          sweep_z(G.KEY, G.ROW0, G.B, G.S, G.LDC, g["mu"], g["ls"]), "the drawn z against the recorded stream")
    assert rel(lat.reshape(G.B, G.S, G.K, Lpad)[:, :, 0, :G.LDC], g["z"]) <= 8 * HALF_ULP + HALF_ULP
    D = 3 * 32 * 32
    for mode, crit in crits().items():
        nll = g["nll_s_" + mode]
        ref = ref_scores(nll, lw, g["la"], g["mu"], g["ls"])
        sc = model.score(x, crit, samples=G.S, key=key, row0=G.ROW0)
        for w in ("recon", "kl_c", "kl_d", "elbo"):
            gate("score %s S=3 %s" % (mode, w), getattr(sc, w), ref[w])
        add = 0.0 if mode == "bce" else -0.5 * D * math.log(2 * math.pi * G.X_SIGMA ** 2)
        lp = model.log_likelihood(x, crit, G.S, key, row0=G.ROW0)
        assert lp.shape == (G.B,) and lp.dtype == torch.float32 and not lp.requires_grad
        gate("log_likelihood %s S=3" % mode, lp, ref["log_px"] + add)
        gate("log_likelihood %s S=3 unnormalised" % mode, model.log_likelihood(x, crit, G.S, key, row0=G.ROW0, normalised=False), ref["log_px"])
        lab = torch.tensor([4, 0, 9, 4], device="cuda")
        nl = np.stack([nll[b, :, int(lab[b])] for b in range(G.B)])[:, :, None]
        refl = ref_scores(nl, lw, g["la"], g["mu"], g["ls"])
        gate("score %s S=3 labelled recon" % mode, model.score(x, crit, label=lab, samples=G.S, key=key, row0=G.ROW0).recon, refl["recon"])
        gate("log_likelihood %s S=3 labelled" % mode, model.log_likelihood(x, crit, G.S, key, label=lab, row0=G.ROW0), refl["log_px"] + add)
    # another row0 is another draw; an int key is the device key of that value
    crit = crits()["bce"]
    assert torch.equal(model.log_likelihood(x, crit, G.S, G.KEY, row0=G.ROW0), model.log_likelihood(x, crit, G.S, key, row0=G.ROW0))
    assert not torch.equal(model.log_likelihood(x, crit, G.S, key, row0=G.ROW0), model.log_likelihood(x, crit, G.S, key, row0=G.ROW0 + 1))


def test_scores_tell_images_classes_and_draws_apart():
    """The fixture's closed-form decoder hardly reads its input (its logits stay below 0.2), so the fixture gate alone would pass with
    the label ignored or a row scored against the wrong image.  Here the same state with the decoder's first layer scaled by 100 (its
    class rows by 300) and its last layer by 30: logits of magnitude ~7, reconstruction terms that differ by ~1e-2 between classes,
    draws and images -- asserted below to be more than 5 x the gate -- and score / log_likelihood against the CPU oracle's decoder
    (held to the reference by tests/test_infer_cpu.py) on the same rows, at the same 1e-3 per image."""
    from oracle import shotvae_oracle as O
    state = dict(CF.make_state(G.NAME, K=G.K))
    w = state["feature_reconstructor.decoder.0.weight"].clone() * 100.0
    w[G.LDC:] *= 3.0
    state["feature_reconstructor.decoder.0.weight"] = w
    state["feature_reconstructor.decoder.15.weight"] = state["feature_reconstructor.decoder.15.weight"] * 30.0
    model = make_model(G.NAME, G.K, "fp32", state).eval()
    x = G.score_inputs()
    key = torch.tensor([G.KEY], dtype=torch.int64, device="cuda")
    mu, ls, la = (t.cpu().numpy() for t in model.encode(x.cuda()))
    z = sweep_z(G.KEY, G.ROW0, G.B, G.S, G.LDC, mu, ls)
    zs = np.concatenate([mu[:, None].astype(np.float64), z], axis=1).astype(np.float32)           # [B, 1 + S, ldc]: z = mu first
    lat = np.concatenate([np.repeat(zs[:, :, None], G.K, axis=2), np.broadcast_to(np.eye(G.K, dtype=np.float32), (G.B, 1 + G.S, G.K, G.K))],
                         axis=3).reshape(-1, G.LDC + G.K)
    with torch.no_grad():
        rec = O.decoder_forward(state, torch.from_numpy(lat)[:, :, None, None], training=False, update=False).numpy()
    nll = nll_rows(rec, np.repeat(x.numpy(), (1 + G.S) * G.K, axis=0), True).reshape(G.B, 1 + G.S, G.K)
    nll_mu, nll_s = nll[:, :1], nll[:, 1:]
    lw = sweep_lw(G.KEY, G.ROW0, G.B, G.S, G.LDC, mu, ls)
    spread = lambda a, axis: float(((a.max(axis=axis) - a.min(axis=axis)) / a.mean(axis=axis)).min())
    figs = (spread(nll_mu[:, 0], 1), spread(nll_s[:, :, 0], 1), spread(nll_mu[:, 0], 0))
    print("FIG amplified decoder: least spread over classes %.3e, draws %.3e, images %.3e; |logit| max %.2f" % (figs + (float(np.abs(rec).max()),)))
    assert min(figs) > 5 * FP32_TOL, "the reference terms are too alike for the gate to tell them apart"
    crit = crits()["bce"]
    for k in range(G.K):
        sc = model.score(x.cuda(), crit, label=torch.full((G.B,), k, dtype=torch.int64, device="cuda"))
        gate("amplified: score label=%d recon" % k, sc.recon, nll_mu[:, 0, k])
    ref0 = ref_scores(nll_mu, None, la, mu, ls)
    gate("amplified: score label=None recon", model.score(x.cuda(), crit).recon, ref0["recon"])
    ref = ref_scores(nll_s, lw, la, mu, ls)
    sc = model.score(x.cuda(), crit, samples=G.S, key=key, row0=G.ROW0)
    gate("amplified: score S=3 recon", sc.recon, ref["recon"])
    gate("amplified: score S=3 elbo", sc.elbo, ref["elbo"])
    gate("amplified: log_likelihood S=3", model.log_likelihood(x.cuda(), crit, G.S, key, row0=G.ROW0), ref["log_px"])
    lab = torch.tensor([4, 0, 9, 4], device="cuda")
    refl = ref_scores(np.stack([nll_s[b, :, int(lab[b])] for b in range(G.B)])[:, :, None], lw, la, mu, ls)
    gate("amplified: score S=3 labelled recon", model.score(x.cuda(), crit, label=lab, samples=G.S, key=key, row0=G.ROW0).recon, refl["recon"])
    gate("amplified: log_likelihood S=3 labelled", model.log_likelihood(x.cuda(), crit, G.S, key, label=lab, row0=G.ROW0), refl["log_px"])


def test_score_equals_the_criterion_on_decode():
    """score(label=y, key=None) is VAECriterion on decode(mu, y) image by image: the batch means of recon, kl_c and kl_d agree with the
    criterion's (and with float64 on the decoder's own logits) to 8 x the error of an fp32 restatement of the same mean, at least
    8 x 2^-24, relative to the float64 value.  Measured on an MI355X, |score - criterion| / |float64| against that allowance: recon
    1.9e-8 of 4.8e-7 (BCE) and 1.4e-7 of 1.0e-6 (MSE), kl_c 3.1e-7 of 8.7e-7, kl_d 1.3e-5 of 1.0e-4 (a sum of ~0.0026 of terms of
    ~0.01: the criterion's fp32 sum and the fp32 restatement both lose those digits)."""
    model, _ = infer_model(G.NAME)
    B = 6
    x = CF.uniform((B, 3, 32, 32), 9710).cuda()
    y = ((torch.arange(B) * 3 + 2) % G.K).cuda()
    mu, ls, la = model.encode(x)
    rec = model.decode(mu, y)
    for mode, crit in crits().items():
        old = [float(v) for v in crit(x, rec, mu, ls, la)]
        sc = model.score(x, crit, label=y)
        new = [float(t.double().mean()) for t in (sc.recon, sc.kl_c, sc.kl_d)]
        r_, x_ = rec.cpu().numpy(), x.cpu().numpy()
        bce, sig = crit.bce_reconstruction, crit.x_sigma
        ref = float(nll_rows(r_, x_, bce, sig).mean())
        e32 = abs(float(nll_rows(r_, x_, bce, sig, np.float32).mean(dtype=np.float32)) - ref) / ref
        kl = ref_scores(np.zeros((B, 1, 1)), None, la.cpu().numpy(), mu.cpu().numpy(), ls.cpu().numpy())
        kl32 = ref_scores(np.zeros((B, 1, 1)), None, la.cpu().numpy(), mu.cpu().numpy(), ls.cpu().numpy(), dtype=np.float32)
        refs = [ref, float(kl["kl_c"].mean()), float(kl["kl_d"].mean())]
        errs = [e32] + [abs(float(kl32[w].mean(dtype=np.float32)) - r0) / abs(r0) for w, r0 in zip(("kl_c", "kl_d"), refs[1:])]
        for name, a, b, r0, e in zip(("recon", "kl_c", "kl_d"), new, old, refs, errs):
            lim = 8.0 * max(e, HALF_ULP)
            print("FIG tie %s %-5s score %.9g criterion %.9g float64 %.9g  |s - c| %.3e |s - f64| %.3e cpu32 %.3e allow %.3e"
                  % (mode, name, a, b, r0, abs(a - b) / abs(r0), abs(a - r0) / abs(r0), e, lim))
            assert abs(a - r0) <= lim * abs(r0) and abs(a - b) <= lim * abs(r0), (mode, name, a, b, r0)


def test_evaluate_scores_does_not_depend_on_the_batching():
    model, _ = infer_model(G.NAME)
    crit = crits()["bce"]
    x = CF.uniform((8, 3, 32, 32), 9711).cuda()
    key = torch.tensor([99], dtype=torch.int64, device="cuda")
    one = S.evaluate_scores(model, crit, [x], samples=2, key=key)
    two = S.evaluate_scores(model, crit, [(x[:3], None), (x[3:], None)], samples=2, key=key)
    assert sorted(one) == ["bits_per_dim", "elbo", "kl_c", "kl_d", "log_px", "recon"] and not model.training
    for k in one:
        e = abs(one[k] - two[k]) / abs(one[k])
        print("FIG evaluate_scores %-12s one batch %.9g, 3 + 5 %.9g: %.3e" % (k, one[k], two[k], e))
        assert e <= FP32_TOL
    assert abs(one["bits_per_dim"] + one["log_px"] / (3072 * math.log(2.0))) < 1e-12
    # per image, and the stream itself bit for bit on the same mu / ls
    whole = model.log_likelihood(x, crit, 2, key)
    parts = torch.cat([model.log_likelihood(x[:3], crit, 2, key), model.log_likelihood(x[3:], crit, 2, key, row0=3)])
    gate("log_likelihood 8 rows against 3 + 5", parts, whole.cpu().numpy())
    mu, ls, _ = model.encode(x)
    Lpad = model._plan.Lpad
    a, lwa = sweep("f32", 8, 2, G.K, G.LDC, Lpad, mu, ls, key)
    b1, lw1 = sweep("f32", 3, 2, G.K, G.LDC, Lpad, mu[:3].contiguous(), ls[:3].contiguous(), key)
    b2, lw2 = sweep("f32", 5, 2, G.K, G.LDC, Lpad, mu[3:].contiguous(), ls[3:].contiguous(), key, row0=3)
    assert np.array_equal(a, np.concatenate([b1, b2])) and np.array_equal(lwa, np.concatenate([lw1, lw2]))
    # without samples: the terms at z = mu, no log_px
    zero = S.evaluate_scores(model, crit, [x])
    sc = model.score(x, crit)
    assert sorted(zero) == ["elbo", "kl_c", "kl_d", "recon"]
    assert all(abs(zero[k] - float(getattr(sc, k).double().mean())) <= 1e-6 * abs(zero[k]) for k in zero)


def test_chunked_equals_unchunked():
    model, _ = infer_model(G.NAME)
    x = G.score_inputs().cuda()
    key = torch.tensor([5], dtype=torch.int64, device="cuda")
    for mode, crit in crits().items():
        whole = model.log_likelihood(x, crit, 2, key)
        for chunk in (27, 1000):                       # 80 rows: 27 + 27 + 26, cut inside an image and inside a sample | one chunk
            gate("log_likelihood %s chunk_rows=%d" % (mode, chunk), model.log_likelihood(x, crit, 2, key, chunk_rows=chunk), whole.cpu().numpy())
        lab = torch.tensor([1, 2, 3, 4], device="cuda")
        gate("log_likelihood %s labelled chunk_rows=3" % mode, model.log_likelihood(x, crit, 2, key, label=lab, chunk_rows=3),
             model.log_likelihood(x, crit, 2, key, label=lab).cpu().numpy())


def test_preactresnet18_runs():
    model, _ = infer_model("preactresnet18")
    x = CF.uniform((3, 3, 32, 32), 9712).cuda()
    key = torch.tensor([1], dtype=torch.int64, device="cuda")
    crit = crits()["bce"]
    sc = model.score(x, crit, samples=2, key=key)
    lp = model.log_likelihood(x, crit, 2, key)
    for t in tuple(sc) + (lp,):
        assert t.shape == (3,) and t.dtype == torch.float32 and bool(torch.isfinite(t).all())
    assert bool((sc.recon > 0).all()) and bool((sc.kl_c >= 0).all()) and bool((lp < 0).all())
    assert per_image(sc.elbo, -(sc.recon.double() + sc.kl_c.double() + sc.kl_d.double()).cpu().numpy()) < 1e-6


def test_bf16_tracks_fp32():
    """wideresnet-28-2, B = 8, S = 2: the per-image recon, elbo and log_px of the bf16 model against the fp32-operand model of the same
    weights, relative <= 5e-3 (the project's bf16 gate on loss scalars).  Measured on an MI355X, BCE / MSE: recon
    1.6e-6 / 6.5e-6, elbo 1.5e-6 / 6.2e-6, log_px 1.8e-6 / 3.1e-6 (kl_c, the encoder's share alone and not gated here: 3.3e-4)"""
    name, B = "wideresnet-28-2", 8
    state = CF.make_state(name, K=G.K)
    m32, m16 = make_model(name, G.K, "fp32", state).eval(), make_model(name, G.K, "bf16", state).eval()
    x = CF.uniform((B, 3, 32, 32), 9713).cuda()
    key = torch.tensor([21], dtype=torch.int64, device="cuda")
    worst = []
    for mode, crit in crits().items():
        a, b = m16.score(x, crit, samples=2, key=key), m32.score(x, crit, samples=2, key=key)
        la_, lb_ = m16.log_likelihood(x, crit, 2, key), m32.log_likelihood(x, crit, 2, key)
        for w, u, v in (("recon", a.recon, b.recon), ("elbo", a.elbo, b.elbo), ("log_px", la_, lb_), ("kl_c", a.kl_c, b.kl_c)):
            e = per_image(u, v.cpu().numpy())
            print("FIG bf16 vs fp32 %s %-6s %.3e" % (mode, w, e))
            if w != "kl_c" and e > BF16_TOL:
                worst.append((mode, w, e))
    assert not worst, worst


def test_log_likelihood_under_graph_capture():
    """log_likelihood with a device key captured into a graph after one eager warm-up call; replayed with another key written to the
    device it equals the eager call with that key, and the model's buffers are what they were"""
    model, _ = infer_model(G.NAME)
    x = G.score_inputs().cuda()
    crit = crits()["bce"]
    key = torch.tensor([11], dtype=torch.int64, device="cuda")
    before = {k: v.clone() for k, v in model.state_dict().items()}
    grad = model.flat_parameters()[1].clone()
    with L.options(deterministic=1):
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            model.log_likelihood(x, crit, 2, key)                # warm-up: weight packs and per-stream caches
        torch.cuda.current_stream().wait_stream(stream)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
            out = model.log_likelihood(x, crit, 2, key)
        for k in (11, 12, 2 ** 40 + 5):
            key.fill_(k)
            graph.replay()
            torch.cuda.synchronize()
            got = out.clone()
            want = model.log_likelihood(x, crit, 2, key)
            assert torch.equal(got, want), "replay with key %d differs from the eager call" % k
        key.fill_(11)
        assert not torch.equal(got, model.log_likelihood(x, crit, 2, key))
    torch.cuda.synchronize()
    after = model.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before), "log_likelihood changed a parameter or a BatchNorm buffer"
    assert all(int(v) == int(before[k]) for k, v in after.items() if k.endswith("num_batches_tracked"))
    assert torch.equal(grad, model.flat_parameters()[1]) and not model._engine._pending
