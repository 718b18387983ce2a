"""The fused glue of the grouped step against the chain it replaces, BIT FOR BIT (torch.equal), both run by the same library on
a real MI355X:

  sv_mix_pack            = sv_mix_lerp x 2 -> torch.cat -> sv_nchw_to_nhwc              (the step's input side)
  sv_sample_fwd_groups   = one sv_sample_fwd per group                                   (the latent neck)
  sv_sample_bwd_groups   = one sv_sample_bwd per group
  sv_shot_loss_step3     = sv_nhwc_to_nchw -> sv_shot_loss_step2 -> sv_nchw_to_nhwc     (the loss stage on the decoder's NHWC logits)
  train_step_grouped with Engine.fused_glue on = the same step with it off              (eager, and captured with a DeviceRng)

No tolerance anywhere a sum has a fixed order: the fused kernels run the device functions of the kernels they replace, so a
difference of one bit is a changed rounding point or a changed summation order.  The one exception is stated where it is made
(test_loss_stage: the loss TERMS in the default mode are sums of float atomics, whose order the hardware chooses -- for both
sides of the comparison)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import shot_vae_amd as S                     # noqa: E402
from oracle import closed_form as CF         # noqa: E402
from oracle import shotvae_oracle as O       # noqa: E402
from shot_vae_amd import _lib as L           # noqa: E402

DT = {"bf16": (L.SV_BF16, torch.bfloat16), "fp32": (L.SV_F32, torch.float32)}
LAM = 0.37


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def lam_args(lam):
    """(host value, device pointer) of a coefficient given as a float or a device scalar"""
    return (0.0, p(lam)) if torch.is_tensor(lam) else (float(lam), None)


# ------------------------------------------------------------------------------------------------ 1. input pack
def _perms(B, g):
    return {"identity": torch.arange(B, device="cuda"), "reversed": torch.arange(B - 1, -1, -1, device="cuda"),
            "random": torch.randperm(B, device="cuda", generator=g)}


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_mix_pack_equals_lerp_cat_convert(B, dtype):
    code, tdt = DT[dtype]
    g = gen(100 + B)
    Cc, H, W, CPAD = 3, 32, 32, 16
    il = torch.rand(B, Cc, H, W, device="cuda", generator=g)
    iu = torch.rand(B, Cc, H, W, device="cuda", generator=g)
    dev_lam = torch.tensor([LAM], device="cuda")
    perms = _perms(B, g)
    for pname_l, pname_u in (("identity", "reversed"), ("reversed", "random"), ("random", "identity")):
        pl, pu = perms[pname_l], perms[pname_u]
        for lam_l, lam_u in ((1.0, 0.0), (0.0, LAM), (LAM, 1.0), (dev_lam, dev_lam)):
            # the chain: two lerps, the concatenation in the launch's group order (1)(3)(2)(4), the layout conversion
            sm, mx = torch.full_like(il, float("nan")), torch.full_like(iu, float("nan"))
            for a, idx, lam, out in ((il, pl, lam_l, sm), (iu, pu, lam_u, mx)):
                L.call("sv_mix_lerp", p(a), p(idx), *lam_args(lam), B, Cc * H * W, 0, p(out), st())
            cat = torch.cat([il, iu, sm, mx])
            ref = torch.full((4 * B, H, W, CPAD), float("nan"), dtype=tdt, device="cuda")
            L.call("sv_nchw_to_nhwc", code, p(cat), 4 * B, Cc, H, W, CPAD, p(ref), st())
            for keep in (False, True):
                out = torch.full((4 * B * H * W * CPAD + 64,), float("nan"), dtype=tdt, device="cuda")     # (+ a guard tail)
                sm2 = torch.full_like(il, float("nan")) if keep else None
                mx2 = torch.full_like(iu, float("nan")) if keep else None
                L.call("sv_mix_pack", code, p(il), p(iu), p(pl), p(pu), *lam_args(lam_l), *lam_args(lam_u), B, Cc, H, W, CPAD,
                       p(out), p(sm2), p(mx2), st())
                got = out[:-64].view(4 * B, H, W, CPAD)
                what = (B, dtype, pname_l, pname_u, lam_l if not torch.is_tensor(lam_l) else "device", keep)
                assert torch.equal(got, ref), what
                assert bool((got[..., Cc:] == 0).all()), what                  # channels 3..15
                assert bool(torch.isnan(out[-64:]).all()), what
                if keep:
                    assert torch.equal(sm2, sm) and torch.equal(mx2, mx), what


# ------------------------------------------------------------------------------------------------ 2. samplers
def _sampler_inputs(B, ldc, K, g):
    n = 4 * B
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    d = dict(mu=r(n, ldc), ls=0.3 * r(n, ldc), la=torch.log_softmax(r(n, K), 1), eps=r(n, ldc),
             u=torch.rand(n, K, device="cuda", generator=g),
             label=torch.randint(0, K, (B,), device="cuda", generator=g), label_mix=torch.randint(0, K, (B,), device="cuda", generator=g))
    return d


def _groups(d, B, lam):
    """the four groups of the grouped step in its launch order (1)(3)(2)(4): one-hot label, Gumbel-softmax, mixed labels, Gumbel-softmax"""
    return [(1, d["label"], None, 0.0), (0, None, None, 0.0), (2, d["label"], d["label_mix"], lam), (0, None, None, 0.0)]


def _table(groups, B, u):
    tab = (L.SvSampleGroup * len(groups))()
    for gi, (mode, label, label_mix, lam) in enumerate(groups):
        t = tab[gi]
        t.mode, t.row0, t.rows = mode, gi * B, B
        if mode == 0:
            t.u = u[gi * B:].data_ptr()
        if label is not None:
            t.label = label.data_ptr()
        if label_mix is not None:
            t.label_mix = label_mix.data_ptr()
        if torch.is_tensor(lam):
            t.lam_dev = lam.data_ptr()
        else:
            t.lam = float(lam)
    return tab


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("ldc,K,Lpad", [(128, 10, 144), (1, 3, 7)])       # the model's sizes; the smallest ldc, a latent with padding
@pytest.mark.parametrize("B", [1, 5])
def test_grouped_samplers_equal_per_group_launches(B, ldc, K, Lpad, dtype):
    code, tdt = DT[dtype]
    g = gen(7 * B + K)
    d = _sampler_inputs(B, ldc, K, g)
    n, TEMP = 4 * B, 0.67
    for lam in (LAM, torch.tensor([LAM], device="cuda")):
        groups = _groups(d, B, lam)
        lat_ref = torch.full((n, Lpad), float("nan"), dtype=tdt, device="cuda")
        cs_ref = torch.full((n, K), float("nan"), device="cuda")
        for gi, (mode, label, label_mix, lm) in enumerate(groups):
            r0 = gi * B
            L.call("sv_sample_fwd", code, p(d["mu"][r0:]), p(d["ls"][r0:]), p(d["la"][r0:]), p(d["eps"][r0:]),
                   p(d["u"][r0:]) if mode == 0 else None, p(label), p(label_mix), *lam_args(lm), mode, TEMP, B, ldc, K, Lpad,
                   p(lat_ref[r0:]), p(cs_ref[r0:]), st())
        lat = torch.full((n, Lpad), float("nan"), dtype=tdt, device="cuda")
        cs = torch.full((n, K), float("nan"), device="cuda")
        L.call("sv_sample_fwd_groups", code, p(d["mu"]), p(d["ls"]), p(d["la"]), p(d["eps"]), _table(groups, B, d["u"]), 4, TEMP,
               ldc, K, Lpad, p(lat), p(cs), st())
        assert not bool(torch.isnan(lat_ref.float()).any()) and not bool(torch.isnan(cs_ref).any())
        assert torch.equal(lat, lat_ref) and torch.equal(cs, cs_ref), (B, ldc, K, dtype, torch.is_tensor(lam))

        # backward: the gradients are ADDED to what the tensors hold
        dl = torch.randn(n, Lpad, device="cuda", generator=g).to(tdt)
        init = [torch.randn(n, w, device="cuda", generator=g) for w in (ldc, ldc, K)]
        ref = [t.clone() for t in init]
        for gi, (mode, _, _, _) in enumerate(groups):
            r0 = gi * B
            L.call("sv_sample_bwd", code, p(dl[r0:]), p(d["ls"][r0:]), p(d["eps"][r0:]), p(cs_ref[r0:]), mode, TEMP, B, ldc, K, Lpad,
                   p(ref[0][r0:]), p(ref[1][r0:]), p(ref[2][r0:]), st())
        got = [t.clone() for t in init]
        L.call("sv_sample_bwd_groups", code, p(dl), p(d["ls"]), p(d["eps"]), p(cs_ref), _table(groups, B, d["u"]), 4, TEMP, ldc, K,
               Lpad, p(got[0]), p(got[1]), p(got[2]), st())
        for name, a, b, i in zip(("d_mu", "d_ls", "d_la"), got, ref, init):
            assert torch.equal(a, b), (name, B, ldc, K, dtype)
            assert name == "d_la" or not torch.equal(a, i), name                 # (something was added)
        # the two reconstructed groups alone, as the step's backward runs it (a prefix of the launch)
        got2 = [t.clone() for t in init]
        L.call("sv_sample_bwd_groups", code, p(dl), p(d["ls"]), p(d["eps"]), p(cs_ref), _table(groups[:2], B, d["u"]), 2, TEMP, ldc, K,
               Lpad, p(got2[0]), p(got2[1]), p(got2[2]), st())
        for a, b, i in zip(got2, ref, init):
            assert torch.equal(a[:2 * B], b[:2 * B]) and torch.equal(a[2 * B:], i[2 * B:])


def test_grouped_sampler_table_is_checked():
    d = _sampler_inputs(2, 4, 3, gen(1))
    lat, cs = torch.empty(8, 8, device="cuda"), torch.empty(8, 3, device="cuda")
    tab = _table(_groups(d, 2, LAM), 2, d["u"])
    tab[2].row0 = 5                                                             # a gap: the groups must tile the rows
    rc = L.lib().sv_sample_fwd_groups(L.SV_F32, p(d["mu"]), p(d["ls"]), p(d["la"]), p(d["eps"]), tab, 4, 0.67, 4, 3, 8, p(lat), p(cs), st())
    assert rc != 0 and b"group 2" in L.lib().sv_last_error()
    rc = L.lib().sv_sample_fwd_groups(L.SV_F32, p(d["mu"]), p(d["ls"]), p(d["la"]), p(d["eps"]), tab, L.MAX_SAMPLE_GROUPS + 1, 0.67, 4, 3, 8,
                                      p(lat), p(cs), st())
    assert rc != 0


# ------------------------------------------------------------------------------------------------ 3. loss stage
def _loss_args(a, o, grads, B, D, K, bce, img_l, img_u, label, pl, pu, terms, scratch):
    for slot in range(4):
        a.mu[slot], a.ls[slot], a.la[slot] = (o[k][slot * B:].data_ptr() for k in ("mu", "ls", "la"))
        a.d_mu[slot], a.d_ls[slot], a.d_la[slot] = (grads[k][slot * B:].data_ptr() for k in ("mu", "ls", "la"))
    a.image_l, a.image_u, a.label_l, a.perm_l, a.perm_u = (t.data_ptr() for t in (img_l, img_u, label, pl, pu))
    a.lam_l, a.lam_u = 0.93, LAM
    a.Bl, a.Bu, a.D, a.K, a.bce, a.n_per_img, a.x_sigma = B, B, D, K, int(bce), img_l[0].numel(), 1.0
    s = O.schedule(10)
    a.sch = L.SvShotSchedule(*[float(s[k]) for k in ("ew", "kl_beta_c", "kl_beta_d", "cmi", "dmi", "pwm", "ucw")])
    a.terms, a.coef, a.tgt = terms.data_ptr(), scratch.data_ptr(), scratch.data_ptr() + 40


@pytest.mark.parametrize("det", [1, 0])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("bce", [True, False])
@pytest.mark.parametrize("B", [2, 5])
def test_loss_stage_on_nhwc_logits_equals_the_nchw_chain(B, bce, dtype, det):
    """terms[12], the six latent gradients of (1) / (3) -- and the six of (2) / (4) -- and the reconstruction gradient with its zero
    padding channels.  det = 1 (SV_OPT_DETERMINISTIC, fixed summation order): everything bit for bit.  det = 0: the gradients bit for
    bit; the loss terms are sums of up to four float atomics (one per block) whose order the hardware picks on BOTH sides, so two
    runs of the SAME kernel may differ in the last bits there: they are held to 4 fp32 ulp (4 * 2^-23 relative), the most a
    reordering of four addends of one sign can move the sum -- the arithmetic itself is the det = 1 case's."""
    code, tdt = DT[dtype]
    D, K, Cc, H, W, ld, ldd = 128, 10, 3, 32, 32, 16, 16
    g = gen(31 * B + int(bce))
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    logits = torch.zeros(2 * B, H, W, ld, dtype=tdt, device="cuda")
    logits[..., :Cc] = (2.0 * r(2 * B, H, W, Cc)).to(tdt)
    logits[..., Cc:] = float("nan")                                   # padding channels of the logits are never read
    o = dict(mu=r(4 * B, D), ls=0.3 * r(4 * B, D), la=torch.log_softmax(r(4 * B, K), 1))
    img_l = torch.rand(B, Cc, H, W, device="cuda", generator=g)
    img_u = torch.rand(B, Cc, H, W, device="cuda", generator=g)
    label = torch.randint(0, K, (B,), device="cuda", generator=g)
    pl, pu = torch.randperm(B, device="cuda", generator=g), torch.randperm(B, device="cuda", generator=g)

    def run(nhwc):
        grads = {k: torch.full_like(v, float("nan")) for k, v in o.items()}
        terms = torch.zeros(12, device="cuda")
        scratch = torch.empty(10 + 4 * B * D + 2 * B * K, device="cuda")
        if nhwc:
            a3 = L.SvShotLossArgs3()
            _loss_args(a3.base, o, grads, B, D, K, bce, img_l, img_u, label, pl, pu, terms, scratch)
            d16 = torch.full((2 * B * H * W * ldd + 64,), float("nan"), dtype=tdt, device="cuda")
            a3.dtype, a3.C, a3.HW, a3.ld_rec, a3.ld_drec = code, Cc, H * W, ld, ldd
            for i in range(2):
                a3.rec[i] = logits[i * B:].data_ptr()
                a3.d_rec[i] = d16[i * B * H * W * ldd:].data_ptr()
            L.call("sv_shot_loss_step3", C.byref(a3), st())
            assert bool(torch.isnan(d16[-64:].float()).all())
            return terms, grads, d16[:-64].view(2 * B, H, W, ldd)
        rec = torch.full((2 * B, Cc, H, W), float("nan"), device="cuda")
        L.call("sv_nhwc_to_nchw", code, p(logits), 2 * B, Cc, H, W, ld, p(rec), st())
        d_rec = torch.full_like(rec, float("nan"))
        a = L.SvShotLossArgs2()
        _loss_args(a, o, grads, B, D, K, bce, img_l, img_u, label, pl, pu, terms, scratch)
        for i in range(2):
            a.rec[i], a.d_rec[i] = rec[i * B:].data_ptr(), d_rec[i * B:].data_ptr()
        L.call("sv_shot_loss_step2", C.byref(a), st())
        d16 = torch.full((2 * B, H, W, ldd), float("nan"), dtype=tdt, device="cuda")
        L.call("sv_nchw_to_nhwc", code, p(d_rec), 2 * B, Cc, H, W, ldd, p(d16), st())
        return terms, grads, d16

    with L.options(deterministic=det):
        t_ref, g_ref, d_ref = run(False)
        t_new, g_new, d_new = run(True)
    torch.cuda.synchronize()
    what = (B, bce, dtype, det)
    assert bool(torch.isfinite(t_ref).all()) and bool(torch.isfinite(d_ref.float()).all())
    if det:
        assert torch.equal(t_new, t_ref), (what, t_new.tolist(), t_ref.tolist())
    else:
        assert bool(((t_new - t_ref).abs() <= 4 * 2.0 ** -23 * t_ref.abs()).all()), (what, t_new.tolist(), t_ref.tolist())
    for k in ("mu", "ls", "la"):
        assert torch.equal(g_new[k], g_ref[k]), (what, k)
    assert torch.equal(d_new, d_ref), what
    assert bool((d_new[..., Cc:] == 0).all()), what
    assert float(d_new[..., :Cc].float().abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 4. the whole step
def _model(name, K, st_, dtype):
    m = S.VariationalAutoEncoder(name, num_input_channels=3, img_size=(32, 32), data_parallel=False, continuous_latent_dim=128,
                                 disc_latent_dim=K, small_input=True, compute_dtype=dtype)
    m.load_state_dict({k: v.detach() for k, v in st_.items()})
    m = m.cuda().train()
    m.rng = "device"
    return m


def _eager_step(fused, dtype, state, batch, K, outputs=False):
    il, ll, iu = batch
    model = _model("wideresnet-10-1", K, state, dtype)
    model._engine.fused_glue = fused
    S.FlatSGD(model).zero_grad()
    elbo, cls = S.VAECriterion(discrete_dim=K).cuda(), S.ClsCriterion()
    torch.manual_seed(11)
    rng = S.DeviceRng("cuda", seed=5)
    out = S.train_step_grouped(model, elbo, cls, None, il, ll, iu, O.schedule(10), device_rng=rng, return_outputs=outputs)
    torch.cuda.synchronize()
    return out, model.flat_parameters()[1].detach().clone()


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_whole_step_is_bit_identical_with_and_without_the_fused_glue(dtype):
    K, B = 10, 8
    state = CF.make_state("wideresnet-10-1", K=K)
    il, ll, iu, _ = CF.make_batch(B, B, K)
    batch = (il.cuda(), ll.cuda(), iu.cuda())
    with L.options(deterministic=1):
        (ls0, lu0), g0 = _eager_step(False, dtype, state, batch, K)
        (ls1, lu1), g1 = _eager_step(True, dtype, state, batch, K)
        full0, _ = _eager_step(False, dtype, state, batch, K, outputs=True)
        full1, g2 = _eager_step(True, dtype, state, batch, K, outputs=True)
    assert bool(torch.isfinite(g0).all()) and float(g0.abs().max()) > 0
    assert torch.equal(ls1, ls0) and torch.equal(lu1, lu0)
    assert torch.equal(g1, g0) and torch.equal(g2, g0)
    # the outputs a caller may ask for are still there, and the same: rec as fp32 NCHW, the two mixed batches
    assert set(full1) == set(full0)
    for k in full0:
        assert torch.equal(full1[k], full0[k]), k
    assert full1["rec1"].shape == (B, 3, 32, 32) and full1["rec1"].dtype == torch.float32


def test_captured_step_is_bit_identical_with_and_without_the_fused_glue():
    """GraphedTrainStep with its DeviceRng: the lambdas reach sv_mix_pack, the sampler table and the loss stage as device pointers,
    and every new entry point is captured (no allocation of its own, no synchronisation)"""
    from shot_vae_amd.train import GraphedTrainStep
    K, B = 10, 8
    state = CF.make_state("wideresnet-10-1", K=K)
    il, ll, iu, _ = CF.make_batch(B, B, K)
    il, ll, iu = il.cuda(), ll.cuda(), iu.cuda()
    res = []
    with L.options(deterministic=1):
        for fused in (False, True):
            model = _model("wideresnet-10-1", K, state, "bf16")
            model._engine.fused_glue = fused
            opt = S.FlatSGD(model, lr=0.05)
            opt.zero_grad()
            elbo, cls = S.VAECriterion(discrete_dim=K).cuda(), S.ClsCriterion()
            torch.manual_seed(13)
            g = GraphedTrainStep(model, elbo, cls, opt, il, ll, iu, O.schedule(10), seed=3, warmup=1)
            for _ in range(2):
                ls, lu = g()
            torch.cuda.synchronize()
            res.append((ls.clone(), lu.clone(), model.flat_parameters()[0].detach().clone()))
    (ls0, lu0, p0), (ls1, lu1, p1) = res
    assert bool(torch.isfinite(p0).all())
    assert torch.equal(ls1, ls0) and torch.equal(lu1, lu0)
    assert torch.equal(p1, p0)
