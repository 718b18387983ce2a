"""Kernel-level parity of the smooth-ELBO entry points (BASELINE config 5: svhn_VAE / mnist_VAE) on a real MI355X:
sv_smooth_latent_fwd / _bwd, sv_smooth_elbo_fwd / _bwd and sv_tanh_to_nchw / _bwd, called directly, against float64 torch on
the CPU built from the formulas of oracle/smooth_oracle.py (forward's latent block, capacity, loss_function).  Gradients are
float64 autograd.  bf16 cases: the reference takes the bf16-rounded inputs; bf16 outputs must equal the bf16 rounding of the
reference within one bf16 ulp.  Every output is pre-filled with NaN, so an element the kernel never writes fails the test."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from shot_vae_amd import _lib as L          # noqa: E402
from oracle import smooth_oracle as SO      # noqa: E402

EPS = SO.EPS
DT = {"f32": (L.SV_F32, torch.float32), "bf16": (L.SV_BF16, torch.bfloat16)}
NAN = float("nan")


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_KEEP = []


def p(t):
    """device pointer of t; keeps t alive until the asynchronous kernel has run"""
    if t is None:
        return None
    _KEEP.append(t)
    if len(_KEEP) > 4096:
        torch.cuda.synchronize()
        del _KEEP[:2048]
    return C.c_void_p(t.data_ptr())


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-20))


def pad16(n):
    return (n + 15) // 16 * 16


def nan_like(shape, dtype):
    return torch.full(shape, NAN, dtype=dtype, device=dev())


def gen(seed):
    return torch.Generator().manual_seed(seed)


def bf16_ulp(x):
    """spacing of bf16 at |x| (8 significant bits); 0 at 0"""
    a = x.abs().double()
    e = torch.floor(torch.log2(a.clamp_min(2.0 ** -126)))
    return torch.where(a > 0, torch.exp2(e - 7), torch.zeros_like(a))


def assert_bf16(got, ref, floor, what):
    """got (bf16) within one bf16 ulp of bf16(ref); `floor` absorbs the fp32 rounding of the kernel's own arithmetic where a
    value is a near-cancellation (an ulp of a value far below the tensor's scale is below that rounding)"""
    got = got.double().cpu()
    r = ref.to(torch.bfloat16).double()
    err = (got - r).abs()
    lim = bf16_ulp(torch.maximum(r.abs(), got.abs())) + floor
    bad = err > lim
    assert not bad.any(), "%s: %d elements beyond 1 bf16 ulp, worst %g (got %g, want %g)" % (
        what, int(bad.sum()), float(err.max()), float(got[bad][0]), float(r[bad][0]))


def check(got, ref, dt, tol, what):
    """fp32: max error relative to the tensor's scale; bf16: the rounding rule above"""
    assert not torch.isnan(got.float().cpu()).any(), what + ": NaN left (element not written)"
    if dt == "bf16" and got.dtype == torch.bfloat16:
        assert_bf16(got, ref, 1e-6 * float(ref.abs().max()), what)
    else:
        e = rel(got, ref)
        assert e < tol, "%s: %g >= %g" % (what, e, tol)


# ------------------------------------------------------------------------------------------------ latent block (heads -> decoder)
LAT_SHAPES = [(1024, 32, 10), (7, 32, 100), (3, 70, 130)]      # production (Dc = 32, Dd = 10, B = 1024); Dd > 64: strided waves


def _latent_inputs(B, Dc, Dd, dt, seed, ties):
    """o = [mean | logvar | logits | pad (NaN: never read)] in the compute dtype, fixed eps and u (incl. u at and next to 0
    and 1), labels; ties: rows whose largest logit repeats at several positions (some more than 64 lanes apart)"""
    g = gen(seed)
    tdt = DT[dt][1]
    ldo = pad16(2 * Dc + Dd)
    o = torch.full((B, ldo), NAN)
    o[:, :Dc] = torch.randn(B, Dc, generator=g)
    o[:, Dc:2 * Dc] = 0.7 * torch.randn(B, Dc, generator=g)
    logits = 1.5 * torch.randn(B, Dd, generator=g)
    if ties:
        for r in range(0, B, 2):
            j = torch.randperm(Dd, generator=g)[:3].sort().values
            logits[r, j[0]] = logits[r, j[1]] = 6.0                    # two equal maxima (6.0: exact in bf16)
            if r % 4 == 0:
                logits[r, j[2]] = 6.0                                  # three
        if Dd > 64:
            logits[1, 3] = logits[1, Dd - 2] = 7.0                     # > 64 lanes apart: first maximum in another wave pass
            logits[B - 1, 70] = logits[B - 1, 129 if Dd > 129 else Dd - 1] = 7.0
            logits[B - 1, 5] = 7.0
    o[:, 2 * Dc:2 * Dc + Dd] = logits
    o = o.to(tdt)
    eps = torch.randn(B, Dc, generator=g)
    u = torch.rand(B, Dd, generator=g)
    edge = torch.tensor([0.0, 1e-30, 1e-7, 0.5, 1.0 - 2 ** -24, 1.0 - 2 ** -23])
    u.view(-1)[:edge.numel()] = edge
    u.view(-1)[-edge.numel():] = edge.flip(0)
    label = torch.randint(0, Dd, (B,), generator=g)
    return o, eps, u, label, ldo


def _latent_ref(o, eps, u, label, Dc, Dd, T, training, sample_grad=False):
    """oracle/smooth_oracle.py forward, latent block, float64: (mean, logvar, alpha, gs, latent); o: float64 [B][2Dc+Dd]"""
    mean, logvar, logits = o[:, :Dc], o[:, Dc:2 * Dc], o[:, 2 * Dc:2 * Dc + Dd]
    alpha = F.softmax(logits, dim=1)
    z = mean + torch.exp(0.5 * logvar) * eps if training else mean
    if training:
        g = -torch.log(-torch.log(u + EPS) + EPS)
        gs = F.softmax((torch.log(alpha + EPS) + g) / T, dim=1)
    else:
        gs = F.one_hot(alpha.argmax(1), Dd).double()                  # torch.argmax: the FIRST maximum
    if label is not None:
        c = F.one_hot(label, Dd).double()
    else:
        c = gs if sample_grad else gs.detach()
    return mean, logvar, alpha, gs, torch.cat([z, c], 1)


@pytest.mark.parametrize("B,Dc,Dd", LAT_SHAPES)
@pytest.mark.parametrize("has_label", [True, False])
@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_smooth_latent_fwd_against_float64(dt, training, has_label, B, Dc, Dd):
    code, tdt = DT[dt]
    d, T = dev(), 0.67
    o, eps, u, label, ldo = _latent_inputs(B, Dc, Dd, dt, 11 + B + Dd, ties=not training)
    Lpad = pad16(Dc + Dd)
    lab = label if has_label else None
    outs = dict(mean=nan_like((B, Dc), torch.float32), logvar=nan_like((B, Dc), torch.float32),
                alpha=nan_like((B, Dd), torch.float32), gs=nan_like((B, Dd), torch.float32),
                latent=nan_like((B, Lpad), tdt), latent32=nan_like((B, Dc + Dd), torch.float32))
    od, ed, ud = o.to(d), eps.to(d), u.to(d)
    ld = lab.to(d) if lab is not None else None
    L.call("sv_smooth_latent_fwd", code, p(od), ldo, p(ed) if training else None, p(ud) if training else None, p(ld), T,
           training, B, Dc, Dd, Lpad, p(outs["mean"]), p(outs["logvar"]), p(outs["alpha"]), p(outs["gs"]), p(outs["latent"]),
           p(outs["latent32"]), st())
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in outs.items()}
    for k, v in got.items():
        assert not torch.isnan(v.float()).any(), k + ": NaN left (element not written)"
    q = o[:, :2 * Dc + Dd].double()                                       # the bf16-rounded operands, upcast
    mean, logvar, alpha, gs, lat = _latent_ref(q, eps.double(), u.double(), lab, Dc, Dd, T, training)
    assert torch.equal(got["mean"].double(), mean) and torch.equal(got["logvar"].double(), logvar)      # plain copies
    # tolerances: observed worst error on an MI355X in brackets
    check(got["alpha"], alpha, "f32", 1e-6, "alpha")               # [1.4e-7]
    if training:
        # [3.2e-6] Gumbel path: 1/T amplifies the rounding of -log(-log(u + EPS) + EPS); at u = 1 - 2^-24 the fp32 sum u + EPS
        # drops EPS, which moves g by ~2e-5 relative
        check(got["gs"], gs, "f32", 2e-5, "gs")
    else:
        assert torch.equal(got["gs"].double(), gs), "eval mode: gs must be one_hot(first argmax of alpha)"
    check(got["latent32"][:, :Dc], lat[:, :Dc], "f32", 1e-6, "latent32 z")           # [7.8e-8]
    check(got["latent32"][:, Dc:], lat[:, Dc:], "f32", 2e-5, "latent32 c")           # [3.2e-6] (= gs)
    check(got["latent"][:, :Dc], lat[:, :Dc], dt, 1e-6, "latent z")                  # [5.4e-8; bf16: 1 ulp]
    check(got["latent"][:, Dc:Dc + Dd], lat[:, Dc:], dt, 2e-5, "latent c")           # [3.2e-6; bf16: 1 ulp]
    assert torch.equal(got["latent"][:, Dc + Dd:].float(), torch.zeros(B, Lpad - Dc - Dd)), "latent pad columns must be 0"


@pytest.mark.parametrize("B,Dc,Dd", LAT_SHAPES)
@pytest.mark.parametrize("null", [None, "dmean", "dlogvar", "dalpha"])
@pytest.mark.parametrize("sample_path", [0, 1])
@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_smooth_latent_bwd_against_float64_autograd(dt, training, sample_path, null, B, Dc, Dd):
    code, tdt = DT[dt]
    d = dev()
    T = 0.67 if null in (None, "dlogvar") else 1.5
    o, eps, u, label, ldo = _latent_inputs(B, Dc, Dd, dt, 29 + B + Dd, ties=False)
    Lpad = pad16(Dc + Dd)
    g = gen(97 + Dd)
    dlat = torch.randn(B, Lpad, generator=g)
    dlat[:, Dc + Dd:] = NAN                                             # pad columns: garbage that must not leak
    dlat = dlat.to(tdt)
    up = {k: torch.randn(B, n, generator=g) for k, n in (("dmean", Dc), ("dlogvar", Dc), ("dalpha", Dd))}
    if null is not None:
        up[null] = None
    # reference forward in float64; the kernel gets its saved tensors (logvar, alpha, gs) rounded to fp32
    x = o[:, :2 * Dc + Dd].double().requires_grad_(True)
    lab = None if sample_path else label
    mean, logvar, alpha, gs, lat = _latent_ref(x, eps.double(), u.double(), lab, Dc, Dd, T, training, sample_grad=True)
    loss = (lat * dlat[:, :Dc + Dd].double()).sum()
    for k, t in (("dmean", mean), ("dlogvar", logvar), ("dalpha", alpha)):
        if up[k] is not None:
            loss = loss + (t * up[k].double()).sum()
    want, = torch.autograd.grad(loss, x)
    d_o = nan_like((B, ldo), tdt)
    L.call("sv_smooth_latent_bwd", code, p(dlat.to(d)), Lpad, p(None if up["dmean"] is None else up["dmean"].to(d)),
           p(None if up["dlogvar"] is None else up["dlogvar"].to(d)), p(None if up["dalpha"] is None else up["dalpha"].to(d)),
           p(logvar.detach().float().to(d)), p(eps.to(d)) if training else None, p(alpha.detach().float().to(d)),
           p(gs.detach().float().to(d)), T, training, sample_path, B, Dc, Dd, p(d_o), ldo, st())
    torch.cuda.synchronize()
    got = d_o.cpu()
    check(got[:, :Dc], want[:, :Dc], dt, 1e-6, "d_mean")                        # [6.9e-8]
    check(got[:, Dc:2 * Dc], want[:, Dc:2 * Dc], dt, 1e-6, "d_logvar")          # [1.1e-7]
    check(got[:, 2 * Dc:2 * Dc + Dd], want[:, 2 * Dc:], dt, 2e-6, "d_logits")   # [2.4e-7] (incl. the Gumbel path)
    assert torch.equal(got[:, 2 * Dc + Dd:].float(), torch.zeros(B, ldo - 2 * Dc - Dd)), "d_o pad columns must be 0"


# ------------------------------------------------------------------------------------------------ the trainer's loss
def _sched(cont, disc, alpha_cls, steps):
    return L.SvSmoothSchedule(*[float(v) for v in cont], *[float(v) for v in disc], float(alpha_cls), float(steps))


def _loss64(data, recon, mean, logvar, alpha, steps, label, cont, disc, cls_alpha):
    """oracle/smooth_oracle.py loss_function in float64 -> (total, raw terms t[0..3], weighted parts, kl_c, kl_d, C_c, C_d)"""
    B = data.shape[0]
    npix = data[0].numel()
    recon_loss = F.mse_loss(recon.reshape(B, npix), data.reshape(B, npix)) * npix
    kl_c = (-0.5 * (1 + logvar - mean.pow(2) - logvar.exp())).mean(0).sum()
    cc = SO.capacity(cont, steps)
    cont_loss = cont[3] * torch.abs(cc - kl_c)
    D = alpha.shape[1]
    negent = (alpha * torch.log(alpha + EPS)).sum(1).mean(0)
    kl_d = math.log(D) + negent
    cd = SO.capacity(disc, steps, math.log(D))
    disc_loss = disc[3] * torch.abs(cd - kl_d)
    bce = F.binary_cross_entropy(alpha, F.one_hot(label, D).double()) if label is not None else torch.zeros((), dtype=torch.float64)
    cls = cls_alpha * bce
    total = recon_loss + cont_loss + disc_loss + cls
    return total, (recon_loss, kl_c, negent, bce), (recon_loss, cont_loss, disc_loss, cls), kl_c, kl_d, cc, cd


def _run_elbo(data, rec, mean, logvar, alpha, label, sch, steps_dev, gout):
    """sv_smooth_elbo_fwd (terms zeroed first, as the caller must) + sv_smooth_elbo_bwd -> CPU tensors"""
    d = dev()
    B, Dc, Dd = data.shape[0], mean.shape[1], alpha.shape[1]
    dd, rd, md, vd, ad = (t.to(d).contiguous() for t in (data, rec, mean, logvar, alpha))
    ld = label.to(d) if label is not None else None
    terms = torch.zeros(9, device=d)
    coef = nan_like((4,), torch.float32)
    sd = torch.tensor([float(steps_dev)], device=d) if steps_dev is not None else None
    L.call("sv_smooth_elbo_fwd", p(dd), p(rd), data[0].numel(), p(md), p(vd), p(ad), p(ld), B, Dc, Dd, C.byref(sch), p(sd),
           p(terms), p(coef), st())
    g = torch.tensor([float(gout)], device=d)
    grads = [nan_like(t.shape, torch.float32) for t in (rec, mean, logvar, alpha)]
    L.call("sv_smooth_elbo_bwd", p(dd), p(rd), data[0].numel(), p(md), p(vd), p(ad), p(ld), B, Dc, Dd, p(coef), p(g),
           *[p(t) for t in grads], st())
    torch.cuda.synchronize()
    return terms.cpu(), coef.cpu(), [t.cpu() for t in grads]


def _elbo_inputs(B, shape, Dc, Dd, seed, has_label):
    g = gen(seed)
    data = torch.rand(B, *shape, generator=g) * 2 - 1
    rec = torch.tanh(data + 0.3 * torch.randn(B, *shape, generator=g))
    mean = 0.5 * torch.randn(B, Dc, generator=g)
    logvar = 0.5 * torch.randn(B, Dc, generator=g)
    alpha = F.softmax(1.2 * torch.randn(B, Dd, generator=g), dim=1)
    label = torch.randint(0, Dd, (B,), generator=g) if has_label else None
    return data, rec, mean, logvar, alpha, label


def _elbo_ref(data, rec, mean, logvar, alpha, label, steps, cont, disc, cls_alpha, gout):
    x = [t.double().requires_grad_(True) for t in (rec, mean, logvar, alpha)]
    total, raw, parts, kl_c, kl_d, cc, cd = _loss64(data.double(), *x, steps, label, cont, disc, cls_alpha)
    grads = torch.autograd.grad(total * gout, x)
    terms = torch.stack([t.detach() for t in raw] + [total.detach()] + [t.detach() for t in parts])
    sgn = lambda v: float(torch.sign(v.detach()))
    coef = torch.tensor([1.0, cont[3] * sgn(kl_c - cc), disc[3] * sgn(kl_d - cd), cls_alpha if label is not None else 0.0],
                        dtype=torch.float64)
    return terms, coef, grads, (float(kl_c.detach() - cc), float(kl_d.detach() - cd))


def _check_terms(terms, want, cont, disc, kl_gap, tol):
    """each term against its reference, relative to the magnitudes it is composed of (|C - KL| is a difference)"""
    mag = want.abs().clone()
    mag[6] = cont[3] * (abs(kl_gap[0]) + float(want[1].abs()) + 1.0)
    mag[7] = disc[3] * (abs(kl_gap[1]) + float(want[2].abs()) + 3.0)
    mag[4] = mag[5] + mag[6] + mag[7] + mag[8]
    err = (terms.double() - want).abs() / mag.clamp_min(1e-20)
    assert float(err.max()) < tol, "terms: worst %g at t[%d] (got %s, want %s)" % (
        float(err.max()), int(err.argmax()), terms.tolist(), want.tolist())


IMAGES = {"svhn": (1024, (3, 32, 32)), "mnist": (1024, (1, 32, 32)), "odd": (5, (3, 7, 7))}     # odd: the scalar tail after the 16-byte loads
CONT, DISC = (0.5, 25.0, 20000, 30.0), (0.2, 1.5, 10000, 20.0)
SCHEDULES = {                   # name: (cont, disc, host steps, device steps or None)
    "start": (CONT, DISC, 0, None),
    "mid_ramp": (CONT, DISC, 7000, None),
    "saturated": (CONT, DISC, 60000, None),                           # past cont_iters and disc_iters: C = max
    "logD_cap": (CONT, (0.0, 50.0, 10000, 20.0), 5000, None),         # C_d ramp 25 < disc_max: only the log D cap binds
    "steps_dev": (CONT, DISC, 1e6, 7000),                             # host count deliberately wrong: the device value must win
}


@pytest.mark.parametrize("sched", list(SCHEDULES))
@pytest.mark.parametrize("has_label", [True, False])
@pytest.mark.parametrize("img", list(IMAGES))
def test_smooth_elbo_against_float64_loss_function(img, has_label, sched):
    B, shape = IMAGES[img]
    Dc, Dd, cls_alpha, gout = 32, 10, 1500.0, 0.37
    cont, disc, steps, steps_dev = SCHEDULES[sched]
    data, rec, mean, logvar, alpha, label = _elbo_inputs(B, shape, Dc, Dd, 3 + B + len(sched), has_label)
    true_steps = steps if steps_dev is None else steps_dev
    want_t, want_c, want_g, gap = _elbo_ref(data, rec, mean, logvar, alpha, label, true_steps, cont, disc, cls_alpha, gout)
    assert min(abs(gap[0]), abs(gap[1])) > 1e-2, "test setup: KL too close to a capacity for the sign to be well defined"
    terms, coef, grads = _run_elbo(data, rec, mean, logvar, alpha, label, _sched(cont, disc, cls_alpha, steps), steps_dev, gout)
    _check_terms(terms, want_t, cont, disc, gap, 2e-6)        # [3.8e-7] float atomics of up to 256 blocks: order varies
    assert torch.equal(coef.double(), want_c), (coef, want_c)
    for name, g, w in zip(("d_rec", "d_mean", "d_logvar", "d_alpha"), grads, want_g):
        check(g, w, "f32", 1e-6, name)                                   # [1.9e-7]


def test_smooth_elbo_kl_exactly_at_capacity():
    """mean = logvar = 0, cont_min = 0, steps = 0: KL_c = C_c = 0 exactly; torch's abs backward gives 0 there, so coef[1],
    d_mean and d_logvar are exactly 0"""
    B, shape, Dc, Dd = 64, (3, 8, 8), 32, 10
    data, rec, _, _, alpha, label = _elbo_inputs(B, shape, Dc, Dd, 5, True)
    mean, logvar = torch.zeros(B, Dc), torch.zeros(B, Dc)
    cont, disc = (0.0, 25.0, 20000, 30.0), DISC
    want_t, want_c, want_g, gap = _elbo_ref(data, rec, mean, logvar, alpha, label, 0, cont, disc, 1500.0, 0.37)
    terms, coef, grads = _run_elbo(data, rec, mean, logvar, alpha, label, _sched(cont, disc, 1500.0, 0), None, 0.37)
    assert gap[0] == 0.0 and float(terms[1]) == 0.0 and float(terms[6]) == 0.0
    assert float(coef[1]) == 0.0 and float(want_c[1]) == 0.0
    assert torch.equal(grads[1], torch.zeros(B, Dc)) and torch.equal(grads[2], torch.zeros(B, Dc))
    _check_terms(terms, want_t, cont, disc, gap, 2e-6)
    check(grads[0], want_g[0], "f32", 1e-6, "d_rec")
    check(grads[3], want_g[3], "f32", 1e-6, "d_alpha")


def test_smooth_elbo_saturated_alpha():
    """rows with logits of +-1e3: alpha exactly 0 / 1 in fp32, the hot class at and away from the label.  BCE's logs clamp
    at -100 (F.binary_cross_entropy) and its gradient is (a - y) / max(a (1 - a), 1e-12): single entries reach ~1e11, so
    d_alpha is compared element-wise with a relative tolerance (a max-scaled norm would hide every other entry)"""
    B, shape, Dc, Dd = 40, (1, 8, 8), 32, 10
    data, rec, mean, logvar, _, label = _elbo_inputs(B, shape, Dc, Dd, 8, True)
    g = gen(9)
    logits = 1.2 * torch.randn(B, Dd, generator=g)
    for r in range(0, B, 2):            # even rows saturated: hot == label on r % 4 == 0, hot != label on r % 4 == 2
        hot = int(label[r]) if r % 4 == 0 else (int(label[r]) + 1 + r % 7) % Dd
        logits[r] = -1e3
        logits[r, hot] = 1e3
    alpha = F.softmax(logits, dim=1)
    assert ((alpha == 0) | (alpha == 1)).view(B // 2, 2, Dd)[:, 0].all()
    cont, disc = CONT, DISC
    want_t, want_c, want_g, gap = _elbo_ref(data, rec, mean, logvar, alpha, label, 7000, cont, disc, 1500.0, 0.37)
    terms, coef, grads = _run_elbo(data, rec, mean, logvar, alpha, label, _sched(cont, disc, 1500.0, 7000), None, 0.37)
    bce_clamped = F.binary_cross_entropy(alpha.double(), F.one_hot(label, Dd).double())
    assert abs(float(terms[3]) - float(bce_clamped)) <= 1e-5 * float(bce_clamped)
    _check_terms(terms, want_t, cont, disc, gap, 2e-6)
    assert torch.equal(coef.double(), want_c)
    a, w = grads[3].double(), want_g[3]
    assert float(w.abs().max()) > 1e10                                 # the 1e-12 floor was reached
    scale = float(w.abs()[w.abs() < 1e6].max())                        # the ordinary entries' scale (near-cancellations)
    err = (a - w).abs() / (w.abs() + scale)
    assert float(err.max()) < 1e-5, "d_alpha element-wise: %g" % float(err.max())
    for name, gg, ww in zip(("d_rec", "d_mean", "d_logvar"), grads[:3], want_g[:3]):
        check(gg, ww, "f32", 1e-6, name)


@pytest.mark.parametrize("img", ["svhn", "mnist"])
def test_smooth_elbo_deterministic_mode(img):
    """L.options(deterministic=1): fixed-order reduction slots (B = 1024: more than one block) -- two calls bitwise equal,
    and within the tolerance of the default (atomic) mode"""
    B, shape = IMAGES[img]
    cont, disc, steps, _ = SCHEDULES["mid_ramp"]
    data, rec, mean, logvar, alpha, label = _elbo_inputs(B, shape, 32, 10, 77, True)
    sch = _sched(cont, disc, 1500.0, steps)
    base = _run_elbo(data, rec, mean, logvar, alpha, label, sch, None, 0.37)
    with L.options(deterministic=1):
        r1 = _run_elbo(data, rec, mean, logvar, alpha, label, sch, None, 0.37)
        r2 = _run_elbo(data, rec, mean, logvar, alpha, label, sch, None, 0.37)
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])
    assert all(torch.equal(a, b) for a, b in zip(r1[2], r2[2]))
    want_t, _, _, gap = _elbo_ref(data, rec, mean, logvar, alpha, label, steps, cont, disc, 1500.0, 0.37)
    _check_terms(r1[0], want_t, cont, disc, gap, 2e-6)
    _check_terms(r1[0], base[0].double(), cont, disc, gap, 2e-6)
    assert torch.equal(r1[1], base[1])
    for a, b in zip(r1[2], base[2]):
        check(a, b, "f32", 1e-6, "det vs default gradients")      # [0: the gradient pass has no reduction]


# ------------------------------------------------------------------------------------------------ tanh + NHWC -> NCHW
TANH_CASES = [(1024, 3, 32, 32, 16), (1024, 1, 32, 32, 16),      # the per-pixel backward kernel (C <= 8, ld % 8 == 0)
              (3, 3, 7, 7, 12), (2, 9, 5, 5, 16)]                # the element-wise fallback; B*H*W not a multiple of 256


@pytest.mark.parametrize("B,Cc,H,W,ld", TANH_CASES)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_tanh_to_nchw_against_float64(dt, B, Cc, H, W, ld):
    code, tdt = DT[dt]
    d = dev()
    g = gen(B * Cc + ld)
    f = 1.5 * torch.randn(B, H, W, ld, generator=g)
    f[..., Cc:] = NAN                                                   # pad channels: never read
    f = f.to(tdt)
    out = nan_like((B, Cc, H, W), torch.float32)
    L.call("sv_tanh_to_nchw", code, p(f.to(d)), B, Cc, H, W, ld, p(out), st())
    x = f[..., :Cc].double().requires_grad_(True)
    y = torch.tanh(x).permute(0, 3, 1, 2)
    d_out = torch.randn(B, Cc, H, W, generator=g)
    want, = torch.autograd.grad(y, x, d_out.double())
    d_f = nan_like((B, H, W, ld), tdt)
    L.call("sv_tanh_to_nchw_bwd", code, p(d_out.to(d)), p(out), B, Cc, H, W, ld, p(d_f), st())
    torch.cuda.synchronize()
    check(out.cpu(), y.detach(), "f32", 1e-6, "tanh")                    # [8.2e-8]
    got = d_f.cpu()
    check(got[..., :Cc], want, dt, 1e-6, "d_f")                          # [8.5e-8; bf16: 1 ulp]
    assert torch.equal(got[..., Cc:].float(), torch.zeros(B, H, W, ld - Cc)), "d_f pad channels must be 0"
