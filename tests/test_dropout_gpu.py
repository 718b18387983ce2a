"""Dropout in the WideResNet encoder (drop_rate > 0) on a real MI355X: the mask generator against its numpy restatement, the
forward kernel (values and norm2's statistics) and the masked BatchNorm backward against their definitions, and whole steps
against the CPU oracle whose norm2 inputs are multiplied by the SAME masks (regenerated from the keys each forward recorded;
the oracle files are untouched -- its BatchNorm is wrapped inside the test)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import shot_vae_amd as S                     # noqa: E402
from shot_vae_amd import _lib as L           # noqa: E402
from oracle import closed_form as C          # noqa: E402
from oracle import shotvae_oracle as O       # noqa: E402
from tests import _cases as T                # noqa: E402
from tests.test_dropout_cpu import keep_mask, thr_of      # noqa: E402

P_DROP = 0.3


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def gpu_mask(keys, unit, p, M, Cc):
    """sv_dropout_mask: uint8 [G][M][C] on the device for the int64 device tensor `keys` [G]"""
    G = keys.numel()
    out = torch.empty(G, M, Cc, dtype=torch.uint8, device="cuda")
    L.call("sv_dropout_mask", _vp(keys), unit, thr_of(p), M, Cc, G, _vp(out), _st())
    return out


def make_model(name, K, dtype, st=None, dp=False, p=P_DROP):
    m = S.VariationalAutoEncoder(encoder_name=name, num_input_channels=3, drop_rate=p, img_size=(32, 32),
                                 data_parallel=dp, continuous_latent_dim=128, disc_latent_dim=K,
                                 sample_temperature=0.67, small_input=True, compute_dtype=dtype)
    if st is not None:
        m.load_state_dict({k: v.detach() for k, v in st.items()})
    return m.cuda().train()


# ---------------------------------------------------------------------------------------------------- 1. the generator
def test_mask_kernel_equals_numpy_restatement():
    """>= 1 M elements: two keys (groups = 2), units 0 and 5, C in {32, 64, 128, 160}, bit for bit"""
    keys = torch.tensor([0x0123456789ABCDEF, -0x5EADBEEF12345678], dtype=torch.int64, device="cuda")
    n = 0
    for unit in (0, 5):
        for Cc in (32, 64, 128, 160):
            M = 65536 // Cc + 3
            got = gpu_mask(keys, unit, P_DROP, M, Cc).cpu().numpy()
            for g in range(2):
                want = keep_mask(int(keys[g]), unit, thr_of(P_DROP), M * Cc).reshape(M, Cc)
                assert np.array_equal(got[g].astype(bool), want), (unit, Cc, g)
                n += M * Cc
    assert n >= 1 << 20


def test_mask_keep_fraction_and_independence():
    """keep fraction within 5 sigma of 1 - p over 16 M elements, overall and per channel; masks of different keys / units agree
    at p^2 + (1 - p)^2 within 5 sigma"""
    M, Cc = 131072, 128
    keys = torch.tensor([11, 12], dtype=torch.int64, device="cuda")
    for p in (0.1, 0.3, 0.5):
        m = gpu_mask(keys[:1], 2, p, M, Cc)[0].double()
        n = M * Cc
        s = (p * (1 - p) / n) ** 0.5
        assert abs(float(m.mean()) - (1 - p)) < 5 * s, (p, float(m.mean()))
        sc = (p * (1 - p) / M) ** 0.5
        per = m.mean(0)
        assert float((per - (1 - p)).abs().max()) < 5 * sc, (p, float((per - (1 - p)).abs().max()))
        agree = p * p + (1 - p) * (1 - p)
        sa = (agree * (1 - agree) / n) ** 0.5
        other_key = gpu_mask(keys[1:], 2, p, M, Cc)[0].double()
        other_unit = gpu_mask(keys[:1], 3, p, M, Cc)[0].double()
        for o in (other_key, other_unit):
            a = float((m == o).double().mean())
            assert abs(a - agree) < 5 * sa, (p, a, agree)


# ---------------------------------------------------------------------------------------------------- 2. the kernels
def _fwd(x, keys, unit, p, out, stats, R):
    G, M, Cc = x.shape
    a = L.dropout_args(keys.data_ptr(), unit, p)
    code = L.SV_BF16 if x.dtype == torch.bfloat16 else L.SV_F32
    L.call("sv_dropout_fwd", code, _vp(x), M, Cc, Cc, ctypes.byref(a), _vp(out), _vp(stats), R, G, _st())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("inplace", [False, True])
def test_dropout_fwd_values_and_statistics(dtype, inplace):
    G, M, Cc, R, unit = 3, 4096 + 40, 64, 4, 7
    torch.manual_seed(0)
    x = (torch.randn(G, M, Cc, device="cuda") * 2 + 0.5).to(dtype)
    keys = torch.tensor([5, -6, 7 << 40], dtype=torch.int64, device="cuda")
    x0 = x.clone()
    out = x if inplace else torch.empty_like(x)
    stats = torch.zeros(G, R, 2 * Cc, dtype=torch.float64, device="cuda")
    _fwd(x, keys, unit, P_DROP, out, stats, R)
    torch.cuda.synchronize()
    mask = gpu_mask(keys, unit, P_DROP, M, Cc).bool()
    scale = float(np.float32(1.0 / (1.0 - P_DROP)))
    want = torch.where(mask, (x0.float() * scale).to(dtype), torch.zeros((), dtype=dtype, device="cuda"))
    assert torch.equal(out.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                       want.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))
    s = stats.sum(1)
    y = want.double()
    ref = torch.cat([y.sum(1), (y * y).sum(1)], 1)
    err = float(((s - ref).abs() / ref.abs().clamp_min(1.0)).max())
    assert err < 1e-6, err
    # deterministic mode: the block sums meet in a fixed order -- two runs agree bit for bit, and with the definition
    with L.options(deterministic=1):
        res = []
        for _ in range(2):
            st2 = torch.zeros(G, R, 2 * Cc, dtype=torch.float64, device="cuda")
            o2 = torch.empty_like(x0)
            _fwd(x0, keys, unit, P_DROP, o2, st2, R)
            torch.cuda.synchronize()
            res.append((o2, st2))
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][0], want) and torch.equal(res[1][0], want)
    assert float(((res[0][1].sum(1) - ref).abs() / ref.abs().clamp_min(1.0)).max()) < 1e-6


def _bwd_case(nbranch, dtype, G=2, M=2048, Cc=64, R=4, seed=1):
    torch.manual_seed(seed)
    x = torch.randn(G, M, Cc, device="cuda").to(dtype)
    gs = [torch.randn(G, M, Cc, device="cuda").to(dtype) for _ in range(nbranch)]
    bsums = [torch.randn(G, R, 2 * Cc, dtype=torch.float64, device="cuda") * 30 for _ in range(nbranch)]
    gammas = [torch.rand(Cc, device="cuda") + 0.5 for _ in range(nbranch)]
    mean = torch.randn(G, Cc, device="cuda") * 0.1
    rstd = torch.rand(G, Cc, device="cuda") + 0.5
    return x, gs, bsums, gammas, mean, rstd


def _bwd(code, x, gs, bsums, gammas, mean, rstd, count, R, drop=None):
    G, M, Cc = x.shape
    arr = (L.SvBnBranch * len(gs))()
    dg = [torch.zeros(Cc, device="cuda") for _ in gs]
    db = [torch.zeros(Cc, device="cuda") for _ in gs]
    for k in range(len(gs)):
        arr[k].g, arr[k].bsums, arr[k].gamma = gs[k].data_ptr(), bsums[k].data_ptr(), gammas[k].data_ptr()
        arr[k].dgamma, arr[k].dbeta, arr[k].replicas, arr[k].sparse = dg[k].data_ptr(), db[k].data_ptr(), R, 0
    dx = torch.empty_like(x)
    if drop is None:
        L.call("sv_bn_bwd_apply", code, M, Cc, Cc, _vp(x), _vp(mean), _vp(rstd), float(count), arr, len(gs), None, _vp(dx), G, _st())
    else:
        L.call("sv_bn_bwd_apply_dropout", code, M, Cc, Cc, _vp(x), _vp(mean), _vp(rstd), float(count), arr, len(gs), None,
               _vp(dx), G, ctypes.byref(drop), _st())
    torch.cuda.synchronize()
    return dx, dg, db


@pytest.mark.parametrize("nbranch", [1, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bn_bwd_apply_dropout_equals_plain_times_mask(nbranch, dtype):
    G, M, Cc, R, unit = 2, 2048, 64, 4, 3
    x, gs, bsums, gammas, mean, rstd = _bwd_case(nbranch, dtype, G, M, Cc, R)
    keys = torch.tensor([123456789, -987654321], dtype=torch.int64, device="cuda")
    a = L.dropout_args(keys.data_ptr(), unit, P_DROP)
    code = L.SV_BF16 if dtype == torch.bfloat16 else L.SV_F32
    dx, dg, db = _bwd(code, x, gs, bsums, gammas, mean, rstd, M, R, drop=a)
    # reference: the plain kernel in fp32 on the same (upcast) operands, times mask x scale
    ref, rg, rb = _bwd(L.SV_F32, x.float(), [g.float() for g in gs], bsums, gammas, mean, rstd, M, R)
    mask = gpu_mask(keys, unit, P_DROP, M, Cc).bool()
    want = torch.where(mask, ref * np.float32(1.0 / (1.0 - P_DROP)), torch.zeros((), device="cuda"))
    assert torch.equal(dx == 0, ~mask | (want == 0))
    if dtype == torch.float32:
        ulp = torch.finfo(torch.float32).eps * want.abs().clamp_min(torch.finfo(torch.float32).tiny)
        assert bool(((dx - want).abs() <= ulp).all())
    else:
        d = (dx.float() - want).abs()
        assert bool((d <= want.abs() * 2.0 ** -8 + 1e-30).all()), float((d / want.abs().clamp_min(1e-30)).max())
    for k in range(nbranch):
        assert torch.equal(dg[k], rg[k]) and torch.equal(db[k], rb[k])


# ---------------------------------------------------------------------------------------------------- 3, 9, 10. steps vs oracle
class MaskedOracle:
    """O._bn wrapped: the input of every *.f_block.norm2 is multiplied by the mask (sv_dropout_mask with the key of that forward
    and unit) x scale before the original runs.  keys: one int per oracle forward, in call order."""

    def __init__(self, monkeypatch, plan, keys, p=P_DROP):
        self.units = {un["bn2"].key: i for i, un in enumerate(plan.units)}
        self.first = plan.units[0]["bn2"].key
        self.keys, self.p, self.fwd = list(keys), p, -1
        self.scale = float(np.float32(1.0 / (1.0 - p)))
        orig = O._bn

        def _bn(st, prefix, x, training, update):
            if training and prefix in self.units:
                if prefix == self.first:
                    self.fwd += 1
                B, Cc, H, W = x.shape
                k = torch.tensor([self.keys[self.fwd]], dtype=torch.int64, device="cuda")
                m = gpu_mask(k, self.units[prefix], self.p, B * H * W, Cc)[0].view(B, H, W, Cc).permute(0, 3, 1, 2).cpu()
                x = x * (m.to(x.dtype) * self.scale)
            return orig(st, prefix, x, training, update)

        monkeypatch.setattr(O, "_bn", _bn)

    def used_all(self):
        return self.fwd == len(self.keys) - 1


def _oracle_state(name, K, dt):
    st = O.default_init(name, K=K, seed=5)
    for k in st:
        if st[k].dtype.is_floating_point:
            st[k] = st[k].to(dt)
        if O.is_param(k):
            st[k].requires_grad_(True)
    return st


def _cast(nz, dt):
    return {k: (v.to(dt) if torch.is_tensor(v) and v.dtype.is_floating_point else v) for k, v in nz.items()}


def _compare(model, out, ref, st32, st64, scalars, tensors):
    m = {"scalar": {}, "tensor": {}, "tensor_grad": {}}
    for k in scalars:
        r = float(ref[k])
        m["scalar"][k] = abs(float(out[k]) - r) / max(abs(r), 1e-6)
    for k in tensors:
        m["tensor"][k] = T.rel_err(out[k].float().cpu().numpy(), ref[k].float().numpy())
    grads = {k.replace(".module.", "."): p.grad.detach().float().cpu() for k, p in model.named_parameters()}
    gmax = max(float(st64[k].grad.norm()) for k in st64 if O.is_param(k))
    fa, fb, worst = [], [], (0.0, "")
    for k in st64:
        if not O.is_param(k) or k.endswith("conv0.bias"):
            continue
        a, b = grads[k].double(), st64[k].grad
        fa.append(a.flatten())
        fb.append(b.flatten())
        err = float((a - b).norm()) / max(float(b.norm()), 1e-4 * gmax)
        worst = max(worst, (err, k))
        m["tensor_grad"][k] = err
    fa, fb = torch.cat(fa), torch.cat(fb)
    m["cos"] = float(fa @ fb / fa.norm() / fb.norm())
    m["worst"] = worst
    sd = {k.replace(".module.", "."): v for k, v in model.state_dict().items()}
    m["running"] = max(T.rel_err(sd[k].float().cpu().numpy(), st32[k].detach().float().numpy()) for k in st32
                       if k.endswith("running_mean") or k.endswith("running_var"))
    m["nbt"] = {int(sd[k]) for k in st32 if k.endswith("num_batches_tracked")}
    return m


def _gate(m, dtype, tol_s, tol_t, tol_g, nbt):
    for k, e in m["scalar"].items():
        assert e <= tol_s, (dtype, k, e)
    for k, e in m["tensor"].items():
        assert e < tol_t, (dtype, k, e)
    if dtype == "fp32":
        for k, e in m["tensor_grad"].items():
            assert e < tol_g, (dtype, k, e)
        assert m["running"] < 1e-3, m["running"]
    else:
        assert m["cos"] > 0.93, m["cos"]
        assert m["running"] < 2e-2, m["running"]
    assert m["nbt"] == {nbt}


def _shot_step_vs_masked_oracle(monkeypatch, name, K, Bl, Bu, dtype, seed=3):
    torch.manual_seed(seed)
    il, ll = torch.rand(Bl, 3, 32, 32), torch.randint(0, K, (Bl,))
    iu = torch.rand(Bu, 3, 32, 32)
    nz = O.make_noise(Bl, Bu, K, seed=11)
    nz["lam_l"] = 0.85
    sch = O.schedule(10)
    model = make_model(name, K, dtype, O.default_init(name, K=K, seed=5), dp=True)
    elbo, cls = S.VAECriterion(discrete_dim=K, bce_reconstruction=True).cuda(), S.ClsCriterion()
    S.FlatSGD(model).zero_grad()
    torch.manual_seed(1234)
    with T.rng_for_step(nz):
        out = S.train_step(model, elbo, cls, None, il.cuda(), ll.cuda(), iu.cuda(), sch, return_outputs=True)
    torch.cuda.synchronize()
    keys = [int(k.item()) for k in model.last_dropout_keys]
    assert len(keys) == 4 and len(set(keys)) == 4
    refs = {}
    for dt in (torch.float32, torch.float64):
        mo = MaskedOracle(monkeypatch, model._plan, keys)
        st = _oracle_state(name, K, dt)
        refs[dt] = (st, O.train_step(st, name, il.to(dt), ll, iu.to(dt), _cast(nz, dt), sch, bce=True))
        assert mo.used_all()
        monkeypatch.undo()
    return _compare(model, out, refs[torch.float32][1], refs[torch.float32][0], refs[torch.float64][0], T.SCALARS, T.TENSORS)


@pytest.mark.parametrize("dtype,tol_s,tol_t,tol_g", [("fp32", 1e-3, 1e-3, 1.5e-2), ("bf16", 5e-3, 3e-2, None)])
def test_step_matches_masked_oracle_b64(monkeypatch, dtype, tol_s, tol_t, tol_g):
    """WRN-28-2, B_l = 64 / B_u = 48 (ragged) at drop_rate = 0.3: the gates of test_model_gpu.py::test_step_matches_oracle_b64"""
    m = _shot_step_vs_masked_oracle(monkeypatch, "wideresnet-28-2", 10, 64, 48, dtype)
    print("\n[%s, dropout 0.3] cosine %.5f, worst tensor %.3f (%s)" % (dtype, m["cos"], *m["worst"]))
    _gate(m, dtype, tol_s, tol_t, tol_g, 4)


def test_wide_step_matches_masked_oracle(monkeypatch):
    """WRN-28-10 (160 / 320 / 640 channels: the wide kernels), K = 100, B = 4, fp32 gates"""
    m = _shot_step_vs_masked_oracle(monkeypatch, "wideresnet-28-10", 100, 4, 4, "fp32")
    _gate(m, "fp32", 1e-3, 1e-3, 1.5e-2, 4)


def test_m2_step_matches_masked_oracle(monkeypatch):
    name, K, B = "wideresnet-28-2", 10, 16
    torch.manual_seed(4)
    il, ll, iu, lu = torch.rand(B, 3, 32, 32), torch.randint(0, K, (B,)), torch.rand(B, 3, 32, 32), torch.randint(0, K, (B,))
    nz = O.make_noise(B, B, K, seed=13)
    sch = O.schedule(10)
    model = make_model(name, K, "fp32", O.default_init(name, K=K, seed=5))
    elbo, cls = S.VAECriterion(discrete_dim=K, bce_reconstruction=True).cuda(), S.ClsCriterion()
    S.FlatSGD(model).zero_grad()
    with T.scripted_rng(randn=[nz["eps1"], nz["eps3"]], rand=[nz["u3"]]):
        out = S.m2_train_step(model, elbo, cls, None, il.cuda(), ll.cuda(), iu.cuda(), lu.cuda(), sch, return_outputs=True)
    torch.cuda.synchronize()
    keys = [int(k.item()) for k in model.last_dropout_keys]
    assert len(keys) == 2
    refs = {}
    for dt in (torch.float32, torch.float64):
        mo = MaskedOracle(monkeypatch, model._plan, keys)
        st = _oracle_state(name, K, dt)
        refs[dt] = (st, O.m2_step(st, name, il.to(dt), ll, iu.to(dt), lu, _cast(nz, dt), sch))
        assert mo.used_all()
        monkeypatch.undo()
    scalars = ["recon_l", "klc_l", "kld_l", "recon_u", "klc_u", "kld_u", "disc_post_l", "kl_inference", "loss_sup", "loss_unsup"]
    tensors = ["rec1", "mu1", "ls1", "la1", "rec3", "mu3", "ls3", "la3"]
    m = _compare(model, out, refs[torch.float32][1], refs[torch.float32][0], refs[torch.float64][0], scalars, tensors)
    _gate(m, "fp32", 1e-3, 1e-3, 1.5e-2, 2)


# ---------------------------------------------------------------------------------------------------- 4. grouped = sequential
@pytest.mark.parametrize("B", [8, 128])
def test_grouped_step_equals_sequential_step_with_dropout(B):
    name, K, dtype, tol = "wideresnet-10-1", 10, "fp32", 1e-3
    st = C.make_state(name, K=K)
    m1, m2 = make_model(name, K, dtype, st), make_model(name, K, dtype, st)
    elbo, cls = S.VAECriterion(discrete_dim=K).cuda(), S.ClsCriterion()
    S.FlatSGD(m1).zero_grad()
    S.FlatSGD(m2).zero_grad()
    il, ll, iu, lu = C.make_batch(B, B, K)
    nz = C.make_noise(B, B, K)
    sch = O.schedule(10)
    torch.manual_seed(77)                     # the keys come from the CPU generator, in the reference's positions
    with T.rng_for_step(nz):
        a = S.train_step(m1, elbo, cls, None, il.cuda(), ll.cuda(), iu.cuda(), sch, return_outputs=True, label_u=lu.cuda())
    torch.manual_seed(77)
    with T.rng_for_step(nz):
        b = S.train_step_grouped(m2, elbo, cls, None, il.cuda(), ll.cuda(), iu.cuda(), sch, return_outputs=True,
                                 label_u=lu.cuda())
    torch.cuda.synchronize()
    ka = [int(k.item()) for k in m1.last_dropout_keys]
    kb = m2.last_dropout_keys[0].tolist()              # one batched launch, groups (1)(3)(2)(4)
    assert len(ka) == 4 and kb == [ka[0], ka[2], ka[1], ka[3]]
    for k in T.SCALARS + ["kl_inference"]:
        assert abs(float(a[k]) - float(b[k])) <= tol * max(abs(float(a[k])), 1e-6), (k, float(a[k]), float(b[k]))
    for k in T.TENSORS:
        if k in ("rec2", "rec4"):
            continue
        assert T.rel_err(b[k].float().cpu().numpy(), a[k].float().cpu().numpy()) < tol, k
    ga, gb = m1.flat_parameters()[1].double(), m2.flat_parameters()[1].double()
    assert float((ga - gb).norm() / ga.norm()) < 2e-3
    sa, sb = m1.state_dict(), m2.state_dict()
    for k in sa:
        if k.endswith("running_mean") or k.endswith("running_var"):
            assert T.rel_err(sb[k].float().cpu().numpy(), sa[k].float().cpu().numpy()) < 1e-4, k
        if k.endswith("num_batches_tracked"):
            assert int(sa[k]) == int(sb[k]) == 4, k


# ---------------------------------------------------------------------------------------------------- 5. graph
def test_graphed_step_with_dropout_equals_eager_step():
    """GraphedTrainStep (grouped) at drop_rate = 0.3 against the eager grouped step with the device draws frozen (randn / rand /
    randint return fixed device tensors per shape, as in test_model_gpu.py::test_graphed_step_equals_eager_step)"""
    from shot_vae_amd.train import GraphedTrainStep, DeviceRng, train_step_grouped
    name, K, Bl, Bu = "wideresnet-10-1", 10, 8, 8
    st = C.make_state(name, K=K)
    il, ll, iu, lu = C.make_batch(Bl, Bu, K)
    il, ll, iu = il.cuda(), ll.cuda(), iu.cuda()
    gen = torch.Generator(device="cuda").manual_seed(7)
    frozen = {}
    real = (torch.randn, torch.rand, torch.randint)

    def fixed(kind, fn):
        def f(*a, **kw):
            key = (kind,) + tuple(x if not isinstance(x, torch.Size) else tuple(x) for x in a)
            if key not in frozen:
                kw = {k: v for k, v in kw.items() if k == "dtype"}
                frozen[key] = fn(*a, device="cuda", generator=gen, **kw)
            return frozen[key].clone()
        return f

    torch.randn, torch.rand, torch.randint = fixed("n", real[0]), fixed("u", real[1]), fixed("i", real[2])
    det = L.options(deterministic=1)
    det.__enter__()
    try:
        sch = O.schedule(10)
        elbo, cls = S.VAECriterion(discrete_dim=K).cuda(), S.ClsCriterion()
        m1, m2 = make_model(name, K, "fp32", st), make_model(name, K, "fp32", st)
        m1.rng = m2.rng = "device"
        o1, o2 = S.FlatSGD(m1, lr=0.05), S.FlatSGD(m2, lr=0.05)
        o1.zero_grad()
        o2.zero_grad()
        steps, warm = 2, 2
        rng1 = DeviceRng(il.device, seed=3)
        for i in range(warm + steps):
            if i == warm:
                rng1.refill()
                rng1.counter.zero_()
            train_step_grouped(m1, elbo, cls, o1, il, ll, iu, sch, device_rng=rng1)
        g = GraphedTrainStep(m2, elbo, cls, o2, il, ll, iu, sch, seed=3, warmup=warm, schedule="grouped")
        for _ in range(steps):
            ls, lu_ = g()
        torch.cuda.synchronize()
        assert torch.isfinite(ls).all() and torch.isfinite(lu_).all()
        assert len(m2.last_dropout_keys) == 1 and torch.equal(m2.last_dropout_keys[0], m1.last_dropout_keys[0])
        sa, sb = m1.state_dict(), m2.state_dict()
        for k in sa:
            if sa[k].dtype.is_floating_point:
                assert T.rel_err(sb[k].cpu().numpy(), sa[k].cpu().numpy()) < 2e-6, k
            else:
                assert int(sa[k]) == int(sb[k]) == 4 * (warm + steps), k
    finally:
        det.__exit__(None, None, None)
        torch.randn, torch.rand, torch.randint = real


def test_graph_replays_draw_fresh_keys():
    from shot_vae_amd.train import GraphedTrainStep
    name, K, B = "wideresnet-10-1", 10, 8
    il, ll, iu, lu = C.make_batch(B, B, K)
    model = make_model(name, K, "fp32", C.make_state(name, K=K))
    model.rng = "device"
    elbo, cls = S.VAECriterion(discrete_dim=K).cuda(), S.ClsCriterion()
    opt = S.FlatSGD(model, lr=0.01)
    opt.zero_grad()
    g = GraphedTrainStep(model, elbo, cls, opt, il.cuda(), ll.cuda(), iu.cuda(), O.schedule(10), warmup=1)
    seen = []
    for _ in range(2):
        ls, lu_ = g()
        torch.cuda.synchronize()
        assert torch.isfinite(ls).all() and torch.isfinite(lu_).all()
        seen.append(model.last_dropout_keys[0].clone())
    assert seen[0].numel() == 4 and not torch.equal(seen[0], seen[1])


# ---------------------------------------------------------------------------------------------------- 6. eval, 7. deterministic
def test_eval_forward_ignores_dropout_and_draws_no_key(monkeypatch):
    name, K, B = "wideresnet-28-2", 10, 16
    st = C.make_state(name, K=K)
    m0 = make_model(name, K, "bf16", st, p=0).eval()
    m3 = make_model(name, K, "bf16", st).eval()
    x = torch.rand(B, 3, 32, 32, device="cuda")

    def no_randint(*a, **k):
        raise AssertionError("an eval forward drew a dropout key")

    outs = []
    for m in (m0, m3):
        torch.manual_seed(5)
        with torch.no_grad():
            monkeypatch.setattr(torch, "randint", no_randint)
            outs.append(m(x))
            monkeypatch.undo()
    torch.cuda.synchronize()
    assert m3.last_dropout_keys == []
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_deterministic_mode_dropout_steps_are_bit_identical():
    name, K, B = "wideresnet-28-2", 10, 32
    st = C.make_state(name, K=K)
    il, ll, iu, lu = C.make_batch(B, B, K)
    nz = C.make_noise(B, B, K)
    res = []
    with L.options(deterministic=1):
        for _ in range(2):
            model = make_model(name, K, "bf16", st)
            elbo, cls = S.VAECriterion(discrete_dim=K).cuda(), S.ClsCriterion()
            S.FlatSGD(model).zero_grad()
            torch.manual_seed(9)
            with T.rng_for_step(nz):
                out = S.train_step_grouped(model, elbo, cls, None, il.cuda(), ll.cuda(), iu.cuda(), O.schedule(10),
                                           return_outputs=True)
            torch.cuda.synchronize()
            res.append((float(out["loss_sup"]), float(out["loss_unsup"]), model.flat_parameters()[1].clone()))
    assert res[0][:2] == res[1][:2] and torch.equal(res[0][2], res[1][2])



# ---------------------------------------------------------------------------------------------------- 8. data parallel
# (the N-rank == one-process equivalence of test_dp_gpu.py at drop_rate = 0.3: every rank draws its keys on its own device
#  generator, so rank 0 replaying a rank's device RNG state reproduces that rank's masks)
import json          # noqa: E402
import os            # noqa: E402
import subprocess    # noqa: E402
import sys           # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DP_EQUIV_WORKER = r'''
import os, sys, json, torch
sys.path.insert(0, %r)
import torch.distributed as dist
import shot_vae_amd as S
from shot_vae_amd import dp
from shot_vae_amd import _lib as L
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)
dist.init_process_group("gloo", rank=rank, world_size=world)
K, B = 10, 16
L.call("sv_set_option", L.OPT_DETERMINISTIC, 1)          # fixed summation order: the comparison is down to the exchange


def make():
    torch.manual_seed(3)
    m = S.VariationalAutoEncoder("wideresnet-10-1", num_input_channels=3, drop_rate=0.3, img_size=(32, 32), data_parallel=True,
                                 continuous_latent_dim=128, disc_latent_dim=K, small_input=True, compute_dtype="fp32",
                                 rng="device").cuda().train()
    o = S.FlatSGD(m, lr=0.05, momentum=0.9, weight_decay=5e-4)
    o.zero_grad()
    return m, o


def shard_inputs(r):
    """data shard + noise stream of rank r (what the DP worker seeds itself with)"""
    torch.manual_seed(100 + r); torch.cuda.manual_seed(100 + r)
    il, iu = torch.rand(B, 3, 32, 32, device="cuda"), torch.rand(B, 3, 32, 32, device="cuda")
    return il, torch.randint(0, K, (B,), device="cuda"), iu


elbo, cls = S.VAECriterion(discrete_dim=K).cuda(), S.ClsCriterion()
sch = S.schedule(10)
# ---- the data-parallel run: this rank's shard, one all-reduce, 1/world in the SGD kernel, two steps ------------------------
model, opt = make()
dp.broadcast_parameters(model)
il, ll, iu = shard_inputs(rank)
rng = S.DeviceRng("cuda", seed=0)
for step in range(2):
    S.train_step_grouped(model, elbo, cls, opt, il, ll, iu, sch, distributed=True, device_rng=rng)
p_dp = model._engine.param.detach().clone()
bufs_dp = model._engine.bufs.detach().clone()
res = None
if rank == 0:
    # ---- ONE process over the concatenated shards, each shard with its own BatchNorm statistics: the shards' steps
    #      accumulate into the flat gradient buffer (no update in between), then one SGD step on the mean ----------------
    ref, ropt = make()
    rng2 = S.DeviceRng("cuda", seed=0)
    gens = {}
    for step in range(2):
        lams = rng2.next_lams()                     # both shards of a step use the SAME pair, like the ranks do
        snap = ref._engine.bufs.detach().clone()
        for r in range(world):
            if step == 0:
                gens[r] = shard_inputs(r) + (torch.cuda.get_rng_state(),)
            il_r, ll_r, iu_r, state = gens[r]
            torch.cuda.set_rng_state(state)         # continue rank r's device noise stream where its last step left it

            class Fixed:                            # DeviceRng stand-in: this step's pair, for every shard
                def next_lams(self):
                    return lams
            if r > 0:
                ref._engine.bufs.copy_(snap)        # running statistics are rank-local: rank 0's are compared below
            S.train_step_grouped(ref, elbo, cls, None, il_r, ll_r, iu_r, sch, device_rng=Fixed())
            if r == 0:
                bufs0 = ref._engine.bufs.detach().clone()
            gens[r] = (il_r, ll_r, iu_r, torch.cuda.get_rng_state())
        ref._engine.bufs.copy_(bufs0)
        ropt.step(grad_scale=1.0 / world)
        ropt.zero_grad()
    p_ref = ref._engine.param.detach()
    d = (p_dp - p_ref).abs().max() / p_ref.abs().max()
    db = (bufs_dp - ref._engine.bufs).abs().max() / ref._engine.bufs.abs().max()
    moved = (p_dp - make()[0]._engine.param).abs().max()
    res = {"rel_param_diff": float(d), "rel_buf_diff": float(db), "moved": float(moved)}
    print(json.dumps(res))
dist.barrier()
dist.destroy_process_group()
'''


def _run_two_ranks(script, port0=29600, world=2):
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port0 + os.getpid() % 300), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=560) for p in procs]
    assert all(p.returncode == 0 for p in procs), [o[1][-1500:] for o in outs]
    line = [ln for ln in outs[0][0].splitlines() if ln.startswith("{")][-1]
    return json.loads(line)


@pytest.mark.timeout(900)
def test_two_rank_dropout_step_equals_single_process_over_both_shards(tmp_path):
    script = tmp_path / "equiv.py"
    script.write_text(DP_EQUIV_WORKER % ROOT)
    res = _run_two_ranks(script, port0=30350, world=2)
    assert res["moved"] > 1e-4, res
    assert res["rel_param_diff"] < 1e-5, res
    assert res["rel_buf_diff"] < 1e-5, res
